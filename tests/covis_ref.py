"""A literal restatement of KeyFrame::UpdateConnections (reference: src/KeyFrame.cc:290-380), LocalMapping::KeyFrameCulling
(src/LocalMapping.cc:640-704, with KeyFrame::SetBadFlag src/KeyFrame.cc:454-472 and MapPoint::EraseObservation / SetBadFlag
src/MapPoint.cc:121-178) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:340-383) with dicts, objects and loops.  Culling MUTATES the
objects as the reference does; it deliberately does not use the closed form of include/orbx.h (the set of culled keyframes), so that
the closed form the kernel implements is tested against it.  A std::map<KeyFrame*, ...> is a dict walked in ascending slot."""
import numpy as np

F32, F64 = np.float32, np.float64
KEYFRAME_DTYPE = np.dtype([("id", "<i4"), ("bad", "u1"), ("not_erase", "u1"), ("pad", "u1", (2,)), ("Ow", "<f4", (3,)), ("th_depth", "<f4")])
POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("ref_kf", "<i4"), ("bad", "u1"), ("pad", "u1", (3,))])
OBSERVATION_DTYPE = np.dtype([("kf", "<i4"), ("idx", "<i4"), ("octave", "u1"), ("stereo", "u1"), ("pad", "u1", (2,))])
FEATURE_DTYPE = np.dtype([("point", "<i4"), ("octave", "<i4"), ("depth", "<f4")])
NORMAL_DTYPE = np.dtype([("normal", "<f4", (3,)), ("max_distance", "<f4"), ("min_distance", "<f4"), ("status", "<i4")])
NORMAL_OK, NORMAL_BAD, NORMAL_NO_OBSERVATION, NORMAL_NO_REFERENCE = 0, 1, 2, 3


def build_table(keyframes, points, rows, scale_factors):
    """rows: (point, kf, idx, octave, stereo) in any order -> the table dict of the package's covis_table"""
    rows = sorted(tuple(int(x) for x in r) for r in rows)
    obs = np.zeros(len(rows), OBSERVATION_DTYPE)
    off = np.zeros(len(points) + 1, np.int32)
    for i, (p, k, idx, octv, st) in enumerate(rows):
        obs[i] = (k, idx, octv, 1 if st else 0, (0, 0))
        off[p + 1] += 1
    off = np.cumsum(off).astype(np.int32)
    return {"kf": np.ascontiguousarray(keyframes, KEYFRAME_DTYPE), "pts": np.ascontiguousarray(points, POINT_DTYPE), "obs_off": off, "obs": obs,
            "sf": np.ascontiguousarray(scale_factors, F32)}


def build_queries(query_kf, features):
    fs = [np.ascontiguousarray(f, FEATURE_DTYPE).reshape(-1) for f in features]
    off = np.zeros(len(fs) + 1, np.int32)
    off[1:] = np.cumsum([len(f) for f in fs])
    return {"query_kf": np.ascontiguousarray(query_kf, np.int32), "feat_off": off, "feat": np.concatenate(fs) if fs else np.zeros(0, FEATURE_DTYPE)}


class MapPoint:
    def __init__(self, rec):
        self.bad = bool(rec["bad"])
        self.pos = rec["pos"].copy()
        self.ref_slot = int(rec["ref_kf"])
        self.obs = {}      # KeyFrame -> idx: mObservations
        self.nObs = 0

    def observations(self):
        return sorted(self.obs.items(), key=lambda kv: kv[0].slot)

    def erase_observation(self, kf):   # src/MapPoint.cc:121-151 (mpRefKF is not read by the culling)
        bad = False
        if kf in self.obs:
            self.nObs -= 2 if kf.stereo_of[self.obs[kf]] else 1
            del self.obs[kf]
            if self.nObs <= 2:
                bad = True
        if bad:
            self.set_bad_flag()

    def set_bad_flag(self):            # src/MapPoint.cc:165-178
        obs = dict(self.obs)
        self.bad = True
        self.obs.clear()
        for kf, idx in obs.items():
            kf.erase_map_point_match(idx)


class KeyFrame:
    def __init__(self, slot, rec):
        self.slot = slot
        self.id = int(rec["id"])
        self.not_erase = bool(rec["not_erase"])
        self.th_depth = F32(rec["th_depth"])
        self.Ow = rec["Ow"].copy()
        self.bad = bool(rec["bad"])
        self.to_be_erased = False
        self.map_points = None         # mvpMapPoints: of a query keyframe only
        self.octave_of = {}            # idx -> mvKeysUn[idx].octave, from the observations
        self.stereo_of = {}            # idx -> mvuRight[idx] >= 0
        self.feat = None

    def erase_map_point_match(self, idx):
        if self.map_points is not None and idx < len(self.map_points):
            self.map_points[idx] = None

    def set_bad_flag(self):            # src/KeyFrame.cc:454-472, + mbBad
        if self.id == 0:
            return
        if self.not_erase:
            self.to_be_erased = True
            return
        for mp in list(self.map_points):
            if mp is not None:
                mp.erase_observation(self)
        self.bad = True


def objects(table, queries=None):
    kfs = [KeyFrame(s, table["kf"][s]) for s in range(len(table["kf"]))]
    mps = [MapPoint(table["pts"][p]) for p in range(len(table["pts"]))]
    off, obs = table["obs_off"], table["obs"]
    for p, mp in enumerate(mps):
        for o in range(off[p], off[p + 1]):
            kf = kfs[int(obs["kf"][o])]
            idx = int(obs["idx"][o])
            mp.obs[kf] = idx
            kf.octave_of[idx], kf.stereo_of[idx] = int(obs["octave"][o]), bool(obs["stereo"][o])
            mp.nObs += 2 if obs["stereo"][o] else 1
    if queries is not None:
        for q, s in enumerate(queries["query_kf"]):
            f = queries["feat"][queries["feat_off"][q]:queries["feat_off"][q + 1]]
            kfs[s].feat = f
            kfs[s].map_points = [mps[int(p)] if p >= 0 else None for p in f["point"]]
    return kfs, mps


def update_connections(table, queries, th=15):
    """-> per query (ids list, weights list, counter dict slot -> count)"""
    kfs, _ = objects(table, queries)
    out = []
    for s in queries["query_kf"]:
        me = kfs[s]
        counter = {}
        for mp in me.map_points:
            if mp is None:
                continue
            if mp.bad:
                continue
            for kf, _idx in mp.observations():
                if kf.slot == me.slot:
                    continue
                counter[kf.slot] = counter.get(kf.slot, 0) + 1
        if not counter:
            out.append(([], [], {}))
            continue
        nmax, kmax, pairs = 0, None, []
        for k in sorted(counter):
            if counter[k] > nmax:
                nmax, kmax = counter[k], k
            if counter[k] >= th:
                pairs.append((counter[k], k))
        if not pairs:
            pairs.append((nmax, kmax))
        pairs.sort()
        ids, ws = [], []
        for w, k in pairs:       # push_front
            ids.insert(0, k)
            ws.insert(0, w)
        out.append((ids, ws, counter))
    return out


def keyframe_culling(table, queries, monocular, th_obs=3):
    """-> (n_mps, n_redundant, verdict, point_bad, trace); trace[q]: dict of what the loop saw"""
    kfs, mps = objects(table, queries)
    n_mps, n_red, verdict, trace = [], [], [], []
    for s in queries["query_kf"]:
        kf = kfs[s]
        if kf.id == 0:
            n_mps.append(0); n_red.append(0); verdict.append(0); trace.append({"skipped_far": 0, "level_rejects": 0, "nobs_walked": []})
            continue
        nRedundant, nMPs, far, level_rejects, walked = 0, 0, 0, 0, []
        for i, mp in enumerate(kf.map_points):
            if mp is None:
                continue
            if mp.bad:
                continue
            if not monocular:
                d = F32(kf.feat["depth"][i])
                if d > kf.th_depth or d < 0:
                    far += 1
                    continue
            nMPs += 1
            if mp.nObs > th_obs:
                walked.append(mp.nObs)      # Observations() of the points whose lists the loop walks
                level = int(kf.feat["octave"][i])
                nObs = 0
                for kfi, idx in mp.observations():
                    if kfi is kf:
                        continue
                    if kfi.octave_of[idx] <= level + 1:
                        nObs += 1
                        if nObs >= th_obs:
                            break
                    else:
                        level_rejects += 1
                if nObs >= th_obs:
                    nRedundant += 1
        v = 0
        if float(nRedundant) > 0.9 * float(nMPs):
            kf.set_bad_flag()
            v = 2 if kf.to_be_erased else 1
        n_mps.append(nMPs); n_red.append(nRedundant); verdict.append(v); trace.append({"skipped_far": far, "level_rejects": level_rejects, "nobs_walked": walked})
    return (np.array(n_mps, np.int32), np.array(n_red, np.int32), np.array(verdict, np.int32), np.array([mp.bad for mp in mps], np.uint8), trace)


def update_normal_and_depth(table):
    """The arithmetic host/frame_shim.h's MapPoint::UpdateNormalAndDepth pins, in numpy scalars"""
    kfs, mps = objects(table)
    sf = table["sf"]
    out = np.zeros(len(mps), NORMAL_DTYPE)
    with np.errstate(all="ignore"):
        for p, mp in enumerate(mps):
            if mp.bad:
                out["status"][p] = NORMAL_BAD
                continue
            if not mp.obs:
                out["status"][p] = NORMAL_NO_OBSERVATION
                continue
            ref = kfs[mp.ref_slot] if mp.ref_slot >= 0 else None
            if ref is None or ref not in mp.obs:
                out["status"][p] = NORMAL_NO_REFERENCE
                continue
            normal = [F32(0), F32(0), F32(0)]
            n = 0
            for kf, _idx in mp.observations():
                normali = [F32(mp.pos[k]) - F32(kf.Ow[k]) for k in range(3)]
                s = F64(0)
                for k in range(3):
                    s = s + F64(normali[k]) * F64(normali[k])
                inv = F32(F64(1.0) / np.sqrt(s))
                for k in range(3):
                    normal[k] = F32(F32(normali[k] * inv) + normal[k])
                n += 1
            s = F64(0)
            for k in range(3):
                d = F32(mp.pos[k]) - F32(ref.Ow[k])
                s = s + F64(d) * F64(d)
            dist = F32(np.sqrt(s))
            level = ref.octave_of[mp.obs[ref]]
            mx = F32(dist * F32(sf[level]))
            out["max_distance"][p] = mx
            out["min_distance"][p] = F32(mx / F32(sf[len(sf) - 1]))
            for k in range(3):
                out["normal"][p][k] = F32(F64(normal[k]) * (F64(1.0) / F64(n)))
    return out
