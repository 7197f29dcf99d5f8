"""A literal restatement of Tracking::UpdateLocalMap (reference: src/Tracking.cc:1340-1484: UpdateLocalKeyFrames, UpdateLocalPoints) and
of what SearchLocalPointsHIP (host/ORBmatcher.cc) packs for orbm_search_local_points, with objects, dicts and loops.  It is sequential:
a std::map<KeyFrame*, ...> is a dict walked in ascending slot, a std::set<KeyFrame*> a list in ascending slot, and the marks are
mnTrackReferenceForFrame members compared with the frame's id.  It deliberately shares nothing with the kernels' formulation (minimum
of positions, scans, bit sets)."""
import numpy as np

import covis_ref as R

VIEW_DTYPE = np.dtype([("normal", "<f4", (3,)), ("max_distance", "<f4"), ("min_distance", "<f4"), ("observations", "<i4")])
INFO_DTYPE = np.dtype([("empty_vote", "<i4"), ("n_voted", "<i4"), ("ref_kf", "<i4"), ("ref_votes", "<i4"), ("extension_end", "<i4"), ("launches", "<i4"),
                       ("syncs", "<i4"), ("pad", "<i4")])
WORLDPOINT_DTYPE = np.dtype([("valid", "<i4"), ("wx", "<f4"), ("wy", "<f4"), ("wz", "<f4"), ("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4"),
                             ("max_distance", "<f4"), ("min_distance", "<f4"), ("observations", "<i4")])
END_RAN_OUT, END_LENGTH, END_PARENT = 0, 1, 2
FRAME_ID = 7      # mCurrentFrame.mnId: any value the marks do not start with


class MapPoint:
    def __init__(self, index, rec, view, desc):
        self.index = index
        self.bad = bool(rec["bad"])
        self.pos = rec["pos"]
        self.view = view
        self.desc = desc
        self.observations = {}           # slot -> idx, filled in ascending slot
        self.mnTrackReferenceForFrame = 0
        self.mnLastFrameSeen = 0


class KeyFrame:
    def __init__(self, slot, rec):
        self.slot = slot
        self.bad = bool(rec["bad"])
        self.map_points = []             # GetMapPointMatches()
        self.ordered_covisibles = []     # GetVectorCovisibleKeyFrames()
        self.children = []               # GetChilds(), ascending slot
        self.parent = None
        self.mnTrackReferenceForFrame = 0

    def best_covisibles(self, n):        # src/KeyFrame.cc:165-172
        return self.ordered_covisibles if len(self.ordered_covisibles) < n else self.ordered_covisibles[:n]


def objects(sc):
    t, q = sc["table"], sc["features"]
    mps = [MapPoint(p, t["pts"][p], sc["views"][p], sc["desc"][p]) for p in range(len(t["pts"]))]
    kfs = [KeyFrame(s, t["kf"][s]) for s in range(len(t["kf"]))]
    for p, mp in enumerate(mps):
        for o in range(t["obs_off"][p], t["obs_off"][p + 1]):
            mp.observations[int(t["obs"]["kf"][o])] = int(t["obs"]["idx"][o])
    for s, kf in enumerate(kfs):
        kf.map_points = [mps[int(p)] if p >= 0 else None for p in q["feat"]["point"][q["feat_off"][s]:q["feat_off"][s + 1]]]
        kf.ordered_covisibles = [kfs[int(c)] for c in sc["cov"][s]]
        kf.children = [kfs[int(c)] for c in sorted(sc["children"][s])]
        kf.parent = kfs[int(sc["parent"][s])] if sc["parent"][s] >= 0 else None
    return kfs, mps


def update_local_map(sc):
    """-> dict: frame_points, holder, ext_obs [N]; local_kf; local_pts; pts (WORLDPOINT_DTYPE); mp_desc [m][32]; info (dict); counters"""
    kfs, mps = objects(sc)
    max_keyframes, nbest = sc.get("max_keyframes", 80), sc.get("nbest", 10)
    frame = [mps[int(p)] if p >= 0 else None for p in sc["frame_points"]]      # mCurrentFrame.mvpMapPoints
    local_kfs = [kfs[int(k)] for k in sc["prev_kf"]]                             # mvpLocalKeyFrames of the frame before
    info = {"empty_vote": 0, "n_voted": 0, "ref_kf": -1, "ref_votes": 0, "extension_end": END_RAN_OUT}

    # ---- UpdateLocalKeyFrames (:1376-1484)
    counter = {}
    for i in range(len(frame)):
        if frame[i] is not None:
            mp = frame[i]
            if not mp.bad:
                for slot in mp.observations:
                    counter[slot] = counter.get(slot, 0) + 1
            else:
                frame[i] = None
    if not counter:
        info["empty_vote"] = 1
    else:
        mx, kfmax = 0, None
        local_kfs = []
        for slot in sorted(counter):
            kf = kfs[slot]
            if kf.bad:
                continue
            if counter[slot] > mx:
                mx, kfmax = counter[slot], kf
            local_kfs.append(kf)
            kf.mnTrackReferenceForFrame = FRAME_ID
        first_stage = len(local_kfs)
        info["n_voted"] = first_stage
        j = 0
        while True:
            if j == first_stage:         # itKF == itEndKF, taken before the loop
                break
            if len(local_kfs) > max_keyframes:
                info["extension_end"] = END_LENGTH
                break
            kf = local_kfs[j]
            for neigh in kf.best_covisibles(nbest):
                if not neigh.bad:
                    if neigh.mnTrackReferenceForFrame != FRAME_ID:
                        local_kfs.append(neigh)
                        neigh.mnTrackReferenceForFrame = FRAME_ID
                        break
            for child in kf.children:
                if not child.bad:
                    if child.mnTrackReferenceForFrame != FRAME_ID:
                        local_kfs.append(child)
                        child.mnTrackReferenceForFrame = FRAME_ID
                        break
            parent = kf.parent
            if parent is not None:
                if parent.mnTrackReferenceForFrame != FRAME_ID:
                    local_kfs.append(parent)
                    parent.mnTrackReferenceForFrame = FRAME_ID
                    info["extension_end"] = END_PARENT
                    break                # :1473: leaves the loop over the keyframes
            j += 1
        if kfmax is not None:
            info["ref_kf"], info["ref_votes"] = kfmax.slot, mx

    # ---- UpdateLocalPoints (:1350-1373)
    local_pts = []
    for kf in local_kfs:
        for mp in kf.map_points:
            if mp is None:
                continue
            if mp.mnTrackReferenceForFrame == FRAME_ID:
                continue
            if not mp.bad:
                local_pts.append(mp)
                mp.mnTrackReferenceForFrame = FRAME_ID

    # ---- SearchLocalPoints' first loop (:1291-1307) and SearchLocalPointsHIP's packing
    for mp in frame:
        if mp is not None:               # the bad ones are NULL already
            mp.mnLastFrameSeen = FRAME_ID
    m = len(local_pts)
    pts = np.zeros(m, WORLDPOINT_DTYPE)
    mp_desc = np.zeros((m, 32), np.uint8)
    index = {}
    for j, mp in enumerate(local_pts):
        index[mp.index] = j
        pts["observations"][j] = mp.view["observations"]
        if mp.mnLastFrameSeen == FRAME_ID:
            continue
        if mp.bad:
            continue
        pts["valid"][j] = 1
        pts["wx"][j], pts["wy"][j], pts["wz"][j] = mp.pos
        pts["nx"][j], pts["ny"][j], pts["nz"][j] = mp.view["normal"]
        pts["max_distance"][j], pts["min_distance"][j] = mp.view["max_distance"], mp.view["min_distance"]
        mp_desc[j] = mp.desc
    N = len(frame)
    holder, ext = np.full(N, -1, np.int32), np.zeros(N, np.int32)
    for i, mp in enumerate(frame):
        if mp is not None:
            if mp.index in index:
                holder[i] = index[mp.index]
            else:
                holder[i] = -2
                ext[i] = mp.view["observations"]
    return {"frame_points": np.array([mp.index if mp is not None else -1 for mp in frame], np.int32).reshape(N), "holder": holder, "ext_obs": ext,
            "local_kf": np.array([kf.slot for kf in local_kfs], np.int32).reshape(len(local_kfs)),
            "local_pts": np.array([mp.index for mp in local_pts], np.int32).reshape(m), "pts": pts, "mp_desc": mp_desc, "info": info, "counters": counter}


ARRAYS = ("frame_points", "holder", "ext_obs", "local_kf", "local_pts", "pts", "mp_desc")
INFO_FIELDS = ("empty_vote", "n_voted", "ref_kf", "ref_votes", "extension_end")


def result_bytes(out):
    """every compared byte of a result: the five rule fields of info, then the arrays"""
    return [np.array([out["info"][k] for k in INFO_FIELDS], np.int32).tobytes()] + [np.ascontiguousarray(out[k]).tobytes() for k in ARRAYS]
