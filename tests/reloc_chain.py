"""Tracking::Relocalization (src/Tracking.cc:1486-1648) chained over a synthetic world of tests/reloc_scene.py: the first loop of
the reference whose every stage runs on the device.  Per query frame:

    DetectRelocalizationCandidates                                                      src/Tracking.cc:1493-1496
    per candidate: isBad -> discard; SearchByBoW(0.75); < 15 matches -> discard;        src/Tracking.cc:1515-1536
        else a PnPsolver over the matches (null and bad map points skipped, the
        correspondence -> keypoint table mvKeyPointIndices kept), nCandidates++         src/PnPsolver.cc:67-110
    while candidates are left and none matched, per live candidate:                      src/Tracking.cc:1543-1635
        iterate(5); bNoMore -> discard, nCandidates--                                    :1556-1563
        a pose: mTcw = pose, ALL N mvpMapPoints overwritten (an inlier's match, else null), sFound = the inliers' points  :1566-1583
        PoseOptimization; nGood < 10 -> next candidate                                   :1585-1588
        the optimiser's outliers lose their points (mvbOutlier of an entry WITHOUT a point is stale: it keeps what an
        earlier optimisation left, src/Optimizer.cc:286-288 resets only entries with a point)               :1590-1592
        nGood < 50: SearchByProjection(10, 100); nadditional + nGood >= 50 -> PoseOptimization;             :1595-1601
            30 < nGood < 50: sFound = every point the frame holds, SearchByProjection(3, 64);               :1605-1611
                nGood + nadditional >= 50 -> PoseOptimization, outliers lose their points                   :1614-1621
        nGood >= 50 -> matched                                                            :1628-1632
    no match: mTcw is emptied                                                             :1637-1641

TEST INFRASTRUCTURE.  The bookkeeping above is host code identical for every backend; a backend supplies the five operations
(database query, SearchByBoW, a PnP solver with iterate, PoseOptimization, SearchByProjection against a keyframe).  The minimal sets of
every iterate call come from a generator seeded by (scene seed, keyframe id, call number): the same for every backend.  Every
backend leaves a trace: per stage call what went in and what came out, per candidate and pass the branches taken.

MUTATIONS names deliberately wrong versions of the bookkeeping (Chain(..., mutate=name)); they exist so that the scenes can be shown
to notice them and are never used by a test that compares backends."""
import importlib

import numpy as np

import bow_scene
import pnp_ref
import reloc_scene as RS

PKG = "orb_slam2v2-1_amd"
RANSAC = (0.99, 10, 300, 4, 0.5, 5.991)                 # :1531
MUTATIONS = ("no_index_map", "keep_non_inliers", "drop_best_flags", "sfound_after_drop", "project_with_pnp_pose")


def scene_sets(seed, kf_id, call, n, iterations):
    """the minimal sets of one iterate call (src/PnPsolver.cc:188-201), the same for every backend"""
    rng = np.random.default_rng([int(seed), int(kf_id), int(call)])
    return pnp_ref.draw_sets(n, iterations, lambda lo, hi: int(rng.integers(lo, hi + 1))) if iterations else np.zeros((0, 4), np.int32)


def correspondences(sc, vm):
    """PnPsolver's constructor (src/PnPsolver.cc:79-101): one correspondence per frame keypoint whose match is a map point that is
    not bad -> (corrs, mvKeyPointIndices)"""
    q, m = sc["query"], sc["map"]
    index = np.array([i for i in range(len(vm)) if vm[i] >= 0 and not m["bad"][vm[i]]], np.int64)
    corrs = np.zeros(len(index), pnp_ref.CORR_DTYPE)
    if len(index):
        corrs["w"] = m["pos"][vm[index]]
        corrs["u"], corrs["v"] = q["k"]["x"][index], q["k"]["y"][index]
        corrs["sigma2"] = RS.LEVEL_SIGMA2[q["k"]["octave"][index]]
    return corrs, index


def observations(sc, mp):
    """what Optimizer::PoseOptimization reads of the frame (src/Optimizer.cc:268-345): a monocular edge per entry with a point"""
    q, m = sc["query"], sc["map"]
    import pose_ref
    obs = np.zeros(len(mp), pose_ref.OBS_DTYPE)
    has = mp >= 0
    obs["valid"], obs["u"], obs["v"], obs["ur"] = has, q["k"]["x"], q["k"]["y"], -1.0
    obs["inv_sigma2"] = RS.INV_LEVEL_SIGMA2[q["k"]["octave"]]
    p = m["pos"][np.maximum(mp, 0)]
    obs["wx"], obs["wy"], obs["wz"] = np.where(has, p[:, 0], 0), np.where(has, p[:, 1], 0), np.where(has, p[:, 2], 0)
    return obs


def kf_points(sc, kf, found, dtype):
    """the keyframe's side of SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, ..) (src/ORBmatcher.cc:1487-1498): an entry counts
    when it has a map point that is not bad and not in sAlreadyFound"""
    m = sc["map"]
    mp = kf["mp"]
    ids = np.maximum(mp, 0)
    kp = np.zeros(len(mp), dtype)
    kp["valid"] = (mp >= 0) & ~m["bad"][ids] & ~np.isin(mp, sorted(found))
    kp["wx"], kp["wy"], kp["wz"] = m["pos"][ids, 0], m["pos"][ids, 1], m["pos"][ids, 2]
    kp["max_distance"], kp["min_distance"], kp["angle"] = m["maxd"][ids], m["mind"][ids], kf["k"]["angle"]
    return kp


class Chain:
    def __init__(self, backend, sc, mutate=None):
        assert mutate is None or mutate in MUTATIONS
        self.be, self.sc, self.mutate = backend, sc, mutate
        self.trace = []            # every stage call: dict(stage, pass, cand, kf, in, out)
        self.steps = []            # the decisions: (pass, candidate, branch, value)
        self.script = []           # the run as commands of tests/cpp/reloc_driver.cc: (command, the state it must print)

    def _log(self, stage, p, i, kf, inp, out):
        self.trace.append(dict(stage=stage, **{"pass": p}, cand=i, kf=kf, **{"in": inp}, out=out))

    def _optimize(self, p, i, kid, st):
        obs = observations(self.sc, st["mp"])
        T, out, ngood, info = self.be.optimize(obs, st["Tcw"], st["outlier"])
        self._log("optimize", p, i, kid, dict(obs=obs, Tcw=st["Tcw"].copy(), outlier=st["outlier"].copy()), dict(Tcw=T, outlier=out, ngood=ngood, info=info))
        st["outlier"] = np.asarray(out, np.uint8).copy()               # only entries with a point were rewritten
        if int((obs["valid"] != 0).sum()) >= 3:                          # :364-365 returns before SetPose
            st["Tcw"] = np.asarray(T, np.float32).copy()
        self.script.append(("optimize", dict(n=int(ngood), T=st["Tcw"].copy(), out=st["outlier"].copy())))
        return int(ngood)

    def _project(self, p, i, kid, st, found, th, dist, Tcw=None):
        kf = self.sc["kfs"][kid]
        kp = kf_points(self.sc, kf, found, self.be.KFPOINT_DTYPE)
        holder = np.where(st["mp"] >= 0, -2, -1).astype(np.int32)
        T = st["Tcw"] if Tcw is None else Tcw
        desc = self.sc["map"]["desc"][np.maximum(kf["mp"], 0)]           # pMP->GetDescriptor() (src/ORBmatcher.cc:1529), not the keyframe's own
        n, h = self.be.project(self.sc["query"], kp, desc, T, holder, th, dist)
        self._log("project", p, i, kid, dict(kf=kp, desc=desc, Tcw=T.copy(), holder=holder, th=th, dist=dist), dict(n=n, holder=h))
        new = h >= 0
        st["mp"][new] = kf["mp"][h[new]]
        self.script.append(("project %d %s %d" % (kid, float(np.float32(th)).hex(), dist), dict(n=int(n), mp=st["mp"].copy())))
        return int(n)

    def run(self):
        sc, be, mut = self.sc, self.be, self.mutate
        q = sc["query"]
        N = len(q["k"])
        st = dict(Tcw=None, mp=np.full(N, -1, np.int64), outlier=np.zeros(N, np.uint8))       # the frame: mTcw, mvpMapPoints, mvbOutlier
        step = lambda p, i, what, v=None: self.steps.append((p, i, what, v))   # noqa: E731
        cand = [int(c) for c in be.detect(q["bow"])]
        self._log("detect", -1, -1, -1, dict(bow=list(q["bow"])), dict(candidates=list(cand)))
        res = dict(ok=False, winner=-1, winner_kf=-1, **{"pass": -1}, candidates=cand)
        self.script.append(("detect", dict(ids=list(cand))))
        nK = len(cand)
        if nK == 0:                                                      # :1495
            step(-1, -1, "no_candidates")
            return self._finish(res, st)
        discarded, solvers, matches, index, calls = [False] * nK, [None] * nK, [None] * nK, [None] * nK, [0] * nK
        ncand = 0
        for i, kid in enumerate(cand):
            kf = sc["kfs"][kid]
            if kf["bad"]:                                                # :1518
                discarded[i] = True
                step(-1, i, "kf_bad")
                continue
            n, mq = be.bow(kf, q, sc["map"]["bad"])
            self._log("bow", -1, i, kid, dict(kf=kid), dict(n=n, match=mq))
            vm = np.full(N, -1, np.int64)                                # vpMapPointMatches: per FRAME keypoint the keyframe's point
            sel = mq >= 0
            vm[mq[sel]] = kf["mp"][sel]
            step(-1, i, "bow_matches", int(n))
            self.script.append(("bow %d" % kid, dict(n=int(n), mp=vm.copy())))
            if n < 15:                                                   # :1523
                discarded[i] = True
                step(-1, i, "few_matches")
                continue
            corrs, index[i] = correspondences(sc, vm)
            solvers[i], matches[i] = be.solver(corrs), vm
            self.script.append(("solver %d" % kid, dict(min_inliers=solvers[i].min_inliers, max_iterations=solvers[i].max_iterations, index=index[i].copy())))
            ncand += 1
        match, p = False, 0
        while ncand > 0 and not match:
            live = [i for i in range(nK) if not discarded[i]]
            sets = {i: scene_sets(sc["seed"], cand[i], calls[i], len(index[i]), solvers[i].planned(5)) for i in live}
            answers = None
            if hasattr(be, "iterate_all"):                               # one batched call for the pass, replayed in candidate order
                answers = dict(zip(live, be.iterate_all([solvers[i] for i in live], 5, [sets[i] for i in live])))
            for i in live:
                kid = cand[i]
                sv = solvers[i]
                if mut == "drop_best_flags" and sv.best_flags is not None:
                    sv.best_flags = np.zeros_like(sv.best_flags); sv.best_inliers = 0
                T, no_more, inl, ninl = answers[i] if answers is not None else sv.iterate(5, sets[i])
                calls[i] += 1
                self._log("pnp", p, i, kid, sv.last_in, sv.last or {})
                full = np.zeros(N, np.uint8)
                full[index[i][np.asarray(inl, bool)]] = 1                # vbInliers: one entry per frame keypoint
                self.script.append(("iterate %d 5 %d %s" % (kid, len(sets[i]), " ".join(str(int(x)) for x in np.asarray(sets[i]).ravel())),
                                    dict(found=int(T is not None), no_more=int(bool(no_more)), n=int(ninl), T=None if T is None else np.asarray(T, np.float32), inl=full)))
                if no_more:                                              # :1559
                    discarded[i] = True
                    ncand -= 1
                    step(p, i, "no_more")
                if T is None:
                    continue
                step(p, i, "pose", int(ninl))
                # :1568-1583: the pose and ALL N entries of mvpMapPoints are overwritten
                st["Tcw"] = np.asarray(T, np.float32).copy()
                T_pnp = st["Tcw"].copy()
                vm = matches[i]
                at = np.arange(len(inl)) if mut == "no_index_map" else index[i]
                if mut != "keep_non_inliers":
                    st["mp"][:] = -1
                on = at[np.asarray(inl, bool)]
                st["mp"][on] = vm[on]
                found = set(int(x) for x in vm[on])
                self._log("adopt", p, i, kid, dict(inliers=np.asarray(inl, np.uint8).copy()), dict(Tcw=st["Tcw"].copy(), mp=st["mp"].copy()))
                self.script.append(("adopt %d" % kid, dict(T=st["Tcw"].copy(), mp=st["mp"].copy())))
                ngood = self._optimize(p, i, kid, st)
                step(p, i, "ngood_1", ngood)
                if ngood < 10:                                           # :1587
                    step(p, i, "ngood_lt_10")
                    continue
                st["mp"][st["outlier"] != 0] = -1                        # :1590-1592, over all N: a stale flag meets a null entry
                self.script.append(("drop_outliers", dict(mp=st["mp"].copy())))
                if mut == "sfound_after_drop":
                    found = set(int(x) for x in st["mp"][st["mp"] >= 0])
                if ngood < 50:                                           # :1595
                    nadd = self._project(p, i, kid, st, found, 10.0, 100, T_pnp if mut == "project_with_pnp_pose" else None)
                    step(p, i, "widen", nadd)
                    if nadd + ngood >= 50:                               # :1599
                        ngood = self._optimize(p, i, kid, st)
                        step(p, i, "ngood_2", ngood)
                        if 30 < ngood < 50:                              # :1605
                            found = set(int(x) for x in st["mp"][st["mp"] >= 0])
                            self.script.append(("refound", dict(n=len(found))))
                            nadd = self._project(p, i, kid, st, found, 3.0, 64)
                            step(p, i, "narrow", nadd)
                            if ngood + nadd >= 50:                       # :1614
                                ngood = self._optimize(p, i, kid, st)
                                step(p, i, "ngood_3", ngood)
                                st["mp"][st["outlier"] != 0] = -1
                                self.script.append(("drop_outliers", dict(mp=st["mp"].copy())))
                if ngood >= 50:                                          # :1628
                    match = True
                    res.update(ok=True, winner=i, winner_kf=kid, **{"pass": p})
                    step(p, i, "match", ngood)
                    break
            p += 1
        if not match:                                                    # :1637-1641
            st["Tcw"] = None
            step(p, -1, "lost")
        return self._finish(res, st)

    def _finish(self, res, st):
        res.update(Tcw=None if st["Tcw"] is None else st["Tcw"].copy(), mp=st["mp"].copy(), outlier=st["outlier"].copy(), steps=list(self.steps))
        self.result = res
        return res


def branches(res):
    return [s[2] for s in res["steps"]]


# ---------------------------------------------------------------------------------------------------- the solver state
class RefSolver:
    """PnPsolver's members across iterate calls (mnIterations, mnBestInliers, mvbBestInliers, mBestTcw) around the restatement
    tests/pnp_ref.py: the state machine tests/test_pnp_gpu.py: test_python_solver_iterates_as_the_reference compares with"""

    def __init__(self, corrs, K):
        self.corrs, self.K = np.ascontiguousarray(corrs, pnp_ref.CORR_DTYPE), tuple(float(k) for k in K)
        self.min_inliers, self.max_iterations = pnp_ref.pnp_parameters(len(self.corrs), *RANSAC[:5])
        self.th2 = RANSAC[5]
        self.iterations, self.best_inliers, self.best_flags, self.best_Tcw = 0, 0, None, None
        self.last_in = self.last = None

    def planned(self, k):
        return 0 if len(self.corrs) < self.min_inliers else max(self.max_iterations - self.iterations, int(k))

    def inputs(self, sets):
        return dict(corrs=self.corrs, K=self.K, th2=self.th2, min_inliers=self.min_inliers, max_iterations=self.max_iterations,
                    sets=np.ascontiguousarray(sets, np.int32), iterations_done=self.iterations, prior_best_inliers=self.best_inliers,
                    prior_best_flags=None if self.best_flags is None else self.best_flags.copy())

    def absorb(self, r):
        self.last = r
        self.iterations += int(r["iterations_run"])
        if r["best_iteration"] >= 0:
            self.best_Tcw = np.array(r["best_Tcw"], np.float32).reshape(4, 4)
        self.best_inliers, self.best_flags = int(r["best_inliers"]), np.array(r["best_flags"], np.uint8)
        if r["pose"] == pnp_ref.POSE_REFINED:
            return np.array(r["Tcw"], np.float32).reshape(4, 4), False, np.array(r["inliers"], np.uint8), int(r["refined_inliers"])
        if r["pose"] in (pnp_ref.POSE_BEST, pnp_ref.POSE_PRIOR_BEST):
            return self.best_Tcw.copy(), True, np.array(r["inliers"], np.uint8), int(r["best_inliers"])
        return None, bool(r["no_more"]), np.zeros(len(self.corrs), np.uint8), 0

    def iterate(self, k, sets):
        n = len(self.corrs)
        self.last_in = self.inputs(sets[:self.planned(k)])
        if n < self.min_inliers:                                         # src/PnPsolver.cc:173-177
            self.last = None
            return None, True, np.zeros(n, np.uint8), 0
        return self.absorb(restated_pnp(self.last_in))


_memo = {}


def memo(stage, key, fn):
    """the restatements' results by input bytes: a stage is restated once per distinct input, whichever chain asks"""
    k = (stage, key)
    if k not in _memo:
        _memo[k] = fn()
    return _memo[k]


def pnp_key(a):
    pf = b"" if a["prior_best_flags"] is None else a["prior_best_flags"].tobytes()
    return (a["corrs"].tobytes(), a["K"], a["th2"], a["min_inliers"], a["max_iterations"], a["sets"].tobytes(), a["iterations_done"],
            a["prior_best_inliers"], pf)


def restated_pnp(a):
    return memo("pnp", pnp_key(a), lambda: pnp_ref.ransac(a["corrs"], a["K"], a["th2"], a["min_inliers"], a["max_iterations"], a["sets"],
                                                         a["iterations_done"], a["prior_best_inliers"], a["prior_best_flags"]))


def restated_optimize(obs, Tcw, outlier):
    import pose_ref
    key = (obs.tobytes(), np.asarray(Tcw, np.float32).tobytes(), np.asarray(outlier, np.uint8).tobytes())
    return memo("optimize", key, lambda: pose_ref.pose_optimization(obs, RS.CAM, Tcw, outlier=outlier))


# ---------------------------------------------------------------------------------------------------- backends
class CpuBackend:
    """the restatements: kfdb_ref, the C oracle's SearchByBoW and SearchByProjection, pnp_ref, pose_ref"""
    name = "cpu"

    def __init__(self, sc):
        import kfdb_ref
        import oracle
        self.o, self.sc = oracle, sc
        self.KFPOINT_DTYPE = oracle.KFPOINT_DTYPE
        self.db = kfdb_ref.Session(sc["nwords"])
        for kf in sc["kfs"]:
            self.db.add(kf["id"], kf["bow"])
        self.geom = oracle.grid_geom(RS.W, RS.H)
        self.cam = oracle.Cam(*RS.CAM)

    def detect(self, qbow):
        return self.db.detect_reloc(qbow)[0]

    def bow(self, kf, q, bad):
        nqs, qit, ncs, cit = bow_scene.intersect(kf["fv"], q["fv"])
        qv = ((kf["mp"] >= 0) & ~bad[np.maximum(kf["mp"], 0)]).astype(np.uint8)
        return self.o.search_by_bow(kf["d"], kf["k"]["angle"], qv, q["d"], q["k"]["angle"], None, nqs, qit, ncs, cit, 50, 0, 0.75, True)

    def solver(self, corrs):
        return RefSolver(corrs, RS.K)

    def optimize(self, obs, Tcw, outlier):
        r = restated_optimize(obs, Tcw, outlier)
        return r["Tcw"].copy(), r["outlier"].copy(), r["ngood"], r

    def project(self, q, kp, kf_desc, Tcw, holder, th, dist):
        return self.o.search_by_projection_kf(q["k"], q["d"], self.geom, RS.SF, RS.LOG_SF, self.cam, Tcw, kp, kf_desc, holder, th, dist)


class CpuBatchedBackend(CpuBackend):
    """every live candidate of a pass iterated before the first answer is used, as the batched device call does"""
    name = "cpu-batched"

    def iterate_all(self, solvers, k, sets):
        return [s.iterate(k, x) for s, x in zip(solvers, sets)]


class PerturbedBackend(CpuBackend):
    """the restatement's optimised pose moved by +-1 float ulp in random entries of [R | t]: what a device pose within the
    optimiser's 1-ulp rule may look like to everything that follows"""
    name = "cpu-perturbed"

    def __init__(self, sc, draw):
        super().__init__(sc)
        self.rng = np.random.default_rng([int(sc["seed"]), int(draw)])

    def optimize(self, obs, Tcw, outlier):
        T, out, ng, r = super().optimize(obs, Tcw, outlier)
        if int((obs["valid"] != 0).sum()) >= 3:
            d = self.rng.integers(-1, 2, (3, 4))
            up, dn = np.nextafter(T[:3], np.float32(np.inf)), np.nextafter(T[:3], np.float32(-np.inf))
            T[:3] = np.where(d > 0, up, np.where(d < 0, dn, T[:3]))
        return T, out, ng, r


class GpuSolver:
    """the library's PnPsolver, with what went into its last call kept for the restatement"""

    def __init__(self, pkg, corrs):
        self.so = pkg.PnPsolver(corrs, RS.K)
        self.so.set_ransac_parameters(*RANSAC)
        self.last_in = self.last = None

    best_flags = property(lambda self: self.so.best_flags, lambda self, v: setattr(self.so, "best_flags", v))
    best_inliers = property(lambda self: self.so.best_inliers, lambda self, v: setattr(self.so, "best_inliers", v))

    min_inliers = property(lambda self: self.so.min_inliers)
    max_iterations = property(lambda self: self.so.max_iterations)

    def planned(self, k):
        return self.so.planned(k)

    def before(self, k, sets):
        so = self.so
        self.last_in = dict(corrs=so.corrs, K=so.K, th2=so.th2, min_inliers=so.min_inliers, max_iterations=so.max_iterations,
                            sets=np.ascontiguousarray(sets[:so.planned(k)], np.int32), iterations_done=so.iterations,
                            prior_best_inliers=so.best_inliers, prior_best_flags=None if so.best_flags is None else so.best_flags.copy())
        so.last = None

    def after(self):
        self.last = self.so.last

    def iterate(self, k, sets):
        self.before(k, sets)
        r = self.so.iterate(k, sets)
        self.after()
        return r


class GpuBackend:
    """the library: KeyFrameDatabase, search_by_bow, PnPsolver.iterate, pose_optimization, and SearchByProjection against a keyframe
    as the host class does it: the oracle's projection stage + match_windows"""
    name = "gpu"

    def __init__(self, sc):
        import oracle
        self.pkg = pkg = importlib.import_module(PKG)
        self.o, self.sc = oracle, sc
        self.KFPOINT_DTYPE = oracle.KFPOINT_DTYPE
        self.db = pkg.KeyFrameDatabase(sc["nwords"])
        for kf in sc["kfs"]:
            self.db.add(kf["id"], [w for w, _ in kf["bow"]], [v for _, v in kf["bow"]])
        self.ogeom, self.geom = oracle.grid_geom(RS.W, RS.H), pkg.grid_geom(RS.W, RS.H)
        self.ocam = oracle.Cam(*RS.CAM)

    def detect(self, qbow):
        return self.db.detect_relocalization_candidates([w for w, _ in qbow], [v for _, v in qbow])

    def bow(self, kf, q, bad):
        nqs, qit, ncs, cit = bow_scene.intersect(kf["fv"], q["fv"])
        qv = ((kf["mp"] >= 0) & ~bad[np.maximum(kf["mp"], 0)]).astype(np.uint8)
        return self.pkg.search_by_bow(kf["d"], kf["k"]["angle"], qv, q["d"], q["k"]["angle"], None, nqs, qit, ncs, cit, 50, 0.75, True)

    def solver(self, corrs):
        return GpuSolver(self.pkg, corrs)

    def optimize(self, obs, Tcw, outlier):
        return self.pkg.pose_optimization(obs, RS.CAM, Tcw, outlier)

    def project(self, q, kp, kf_desc, Tcw, holder, th, dist):
        wq = self.o.kf_window_queries(kp, self.ogeom, RS.SF, RS.LOG_SF, self.ocam, Tcw, th)
        return self.pkg.match_windows(q["k"], q["d"], None, self.geom, wq, kf_desc, holder, None, dist, True)


class GpuBatchedBackend(GpuBackend):
    """the live candidates of one pass through ONE PnPsolver.iterate_all call"""
    name = "gpu-batched"

    def iterate_all(self, solvers, k, sets):
        for s, x in zip(solvers, sets):
            s.before(k, x)
        out = self.pkg.PnPsolver.iterate_all([s.so for s in solvers], k, sets)
        for s in solvers:
            s.after()
        return out


_cpu_chains = {}


def cpu_chain(name):
    """the CPU chain of a scene, run once per process and left unchanged; .seconds is that run's wall time"""
    import time
    if name not in _cpu_chains:
        sc = RS.scene(name)
        t0 = time.perf_counter()
        ch = Chain(CpuBackend(sc), sc)
        ch.run()
        ch.seconds = time.perf_counter() - t0
        _cpu_chains[name] = ch
    return _cpu_chains[name]


# ---------------------------------------------------------------------------------------------------- comparing traces
def digest(chain):
    """every stage's outputs and every decision of a run as bytes"""
    parts = []
    for e in chain.trace:
        parts.append(repr((e["stage"], e["pass"], e["cand"], e["kf"])).encode())
        for k in sorted(e["out"]):
            v = e["out"][k]
            if e["stage"] == "pnp":
                if k not in ("Tcw", "best_Tcw", "inliers", "best_flags", "counts", "hit_iteration", "iterations_run", "best_iteration", "best_inliers",
                             "refined_inliers", "no_more", "pose"):
                    continue
            if k == "info":
                continue
            parts.append(k.encode() + (np.ascontiguousarray(v).tobytes() if isinstance(v, np.ndarray) else repr(v).encode()))
    r = chain.result
    parts.append(repr((r["ok"], r["winner"], r["pass"], r["steps"])).encode() + r["mp"].tobytes() + (b"" if r["Tcw"] is None else r["Tcw"].tobytes()))
    return b"|".join(parts)
