"""A literal restatement of the two map-sized loops of LoopClosing with objects, lists and loops: the pose and point correction of
CorrectLoop (reference: src/LoopClosing.cc:444-525, without the UpdateConnections() of :524) and what RunGlobalBundleAdjustment does
after the optimisation (:685-746).  Both MUTATE their objects in the reference's order - a keyframe's SetPose after its point loop, the
queue walk with SetPose when a keyframe is popped - and deliberately do not use the closed forms the kernels implement (a point's owner
as a minimum of positions, the tree's levels), so that those are tested against it.  A std::map<KeyFrame*, ...> is walked in ascending
slot.  cv::Mat arithmetic: terms widened to double, summed left to right, narrowed once (csrc/orbx_cvmath.h); g2o::Sim3 through
tests/essential_ref.py.

MUTATIONS name wrong versions; every one must change the expected output on at least one scene (tests/test_mapcorrect_cpu.py)."""
import numpy as np

from essential_ref import SIM3_DTYPE, inverse, mul, quat_from_R, quat_to_R, smap

F32, F64 = np.float32, np.float64
NORMAL_DTYPE = np.dtype([("normal", "<f4", (3,)), ("max_distance", "<f4"), ("min_distance", "<f4"), ("status", "<i4")])
NORMAL_OK, NORMAL_BAD, NORMAL_NO_OBSERVATION, NORMAL_NO_REFERENCE, NORMAL_UNTOUCHED = 0, 1, 2, 3, 4
SPREAD_UNTOUCHED, SPREAD_GBA, SPREAD_MOVED, SPREAD_UNDEFINED = 0, 1, 2, 3
LOOP_ARRAYS = ("corrected", "non_corrected", "Tiw_new", "Ow_new", "pos", "corrected_ref", "normals")
SPREAD_ARRAYS = ("Tcw_new", "TcwGBA", "kf_marked", "kf_reached", "pos", "status")
MUTATIONS = ("all_observers_corrected", "no_observer_corrected", "last_keyframe_owns", "maps_swapped", "parent_new_pose", "parent_pointers")
LOOP_MUTATIONS, SPREAD_MUTATIONS = MUTATIONS[:4], MUTATIONS[4:]


# ---- cv::Mat on CV_32F -----------------------------------------------------------------------------------------------------------------
def gemm44(a, b):
    d = np.zeros((4, 4), F32)
    for i in range(4):
        for j in range(4):
            s = F64(a[i, 0]) * F64(b[0, j]) + F64(a[i, 1]) * F64(b[1, j])
            s = s + F64(a[i, 2]) * F64(b[2, j])
            s = s + F64(a[i, 3]) * F64(b[3, j])
            d[i, j] = F32(s)
    return d


def gemv3_add(A, x, c):
    """A * x + c: ((a_i0 x_0 + a_i1 x_1) + a_i2 x_2) + c_i"""
    return np.array([F32(((F64(A[i, 0]) * F64(x[0]) + F64(A[i, 1]) * F64(x[1])) + F64(A[i, 2]) * F64(x[2])) + F64(c[i])) for i in range(3)], F32)


def set_pose(Tcw):
    """KeyFrame::SetPose (src/KeyFrame.cc:70-84) -> (Ow, Twc): Ow = -Rwc * tcw as one gemm with alpha = -1"""
    Rwc = Tcw[:3, :3].T
    tcw = Tcw[:3, 3]
    Ow = np.array([F32(((F64(Rwc[i, 0]) * F64(tcw[0]) + F64(Rwc[i, 1]) * F64(tcw[1])) + F64(Rwc[i, 2]) * F64(tcw[2])) * F64(-1.0)) for i in range(3)], F32)
    Twc = np.eye(4, dtype=F32)
    Twc[:3, :3] = Rwc
    Twc[:3, 3] = Ow
    return Ow, Twc


# ---- g2o::Sim3 as (q [1, 4], t [1, 3], s [1]) --------------------------------------------------------------------------------------------
def sim3_of_pose(T):
    """Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0)"""
    return quat_from_R(T[:3, :3].astype(F64)[None]), T[:3, 3].astype(F64)[None], np.ones(1)


def sim3_of_record(r):
    return np.array(r["q"], F64).reshape(1, 4), np.array(r["t"], F64).reshape(1, 3), np.array([r["s"]], F64)


def record_of_sim3(S):
    r = np.zeros(1, SIM3_DTYPE)
    r["q"][0], r["t"][0], r["s"][0] = S[0][0], S[1][0], S[2][0]
    return r[0]


def update_normal(table, p, pos, Ow, octave_of):
    """MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:340-383) of point p at `pos`, the arithmetic host/frame_shim.h pins; Ow [K][3]: every
    keyframe's GetCameraCenter() NOW"""
    out = np.zeros(1, NORMAL_DTYPE)[0]
    off, obs, sf = table["obs_off"], table["obs"], table["sf"]
    lo, hi = int(off[p]), int(off[p + 1])
    if hi == lo:
        out["status"] = NORMAL_NO_OBSERVATION
        return out
    ref = int(table["pts"]["ref_kf"][p])
    if ref < 0 or ref not in [int(k) for k in obs["kf"][lo:hi]]:
        out["status"] = NORMAL_NO_REFERENCE
        return out
    with np.errstate(all="ignore"):
        normal = [F32(0), F32(0), F32(0)]
        n = 0
        for o in range(lo, hi):
            Owi = Ow[int(obs["kf"][o])]
            normali = [F32(pos[k]) - F32(Owi[k]) for k in range(3)]
            s = F64(0)
            for k in range(3):
                s = s + F64(normali[k]) * F64(normali[k])
            inv = F32(F64(1.0) / np.sqrt(s))
            for k in range(3):
                normal[k] = F32(F32(normali[k] * inv) + normal[k])
            n += 1
        s = F64(0)
        for k in range(3):
            d = F32(pos[k]) - F32(Ow[ref][k])
            s = s + F64(d) * F64(d)
        dist = F32(np.sqrt(s))
        mx = F32(dist * F32(sf[octave_of[(p, ref)]]))
        out["max_distance"] = mx
        out["min_distance"] = F32(mx / F32(sf[len(sf) - 1]))
        for k in range(3):
            out["normal"][k] = F32(F64(normal[k]) * (F64(1.0) / F64(n)))
    return out


def correct_loop(table, queries, cur, Tiw, Scw, mutation=None):
    """-> dict of LOOP_ARRAYS.  queries["query_kf"] ascending: the walk order of CorrectedSim3"""
    assert mutation is None or mutation in MUTATIONS
    K, P, Q = len(table["kf"]), len(table["pts"]), len(queries["query_kf"])
    qk = [int(s) for s in queries["query_kf"]]
    curpos = qk.index(int(cur))
    Tiw = np.ascontiguousarray(Tiw, F32)
    Scw_ = sim3_of_record(Scw)
    out = {"corrected": np.zeros(Q, SIM3_DTYPE), "non_corrected": np.zeros(Q, SIM3_DTYPE), "Tiw_new": np.zeros((Q, 4, 4), F32), "Ow_new": np.zeros((Q, 3), F32),
           "pos": table["pts"]["pos"].astype(F32).copy(), "corrected_ref": np.full(P, -1, np.int32), "normals": np.zeros(P, NORMAL_DTYPE)}
    out["normals"]["status"] = NORMAL_UNTOUCHED
    # :448-479
    _, Twc = set_pose(Tiw[curpos])
    corrected, non_corrected = {}, {}
    for q in range(Q):
        if q != curpos:
            Tic = gemm44(Tiw[q], Twc)
            corrected[q] = mul(sim3_of_pose(Tic), Scw_)
        else:
            corrected[q] = Scw_
        non_corrected[q] = sim3_of_pose(Tiw[q])
        out["corrected"][q], out["non_corrected"][q] = record_of_sim3(corrected[q]), record_of_sim3(non_corrected[q])
    # :482-525: the keyframes' camera centres change while the loop runs
    Ow = [table["kf"]["Ow"][k].astype(F32).copy() for k in range(K)]
    octave_of = {}
    for p in range(P):
        for o in range(int(table["obs_off"][p]), int(table["obs_off"][p + 1])):
            octave_of[(p, int(table["obs"]["kf"][o]))] = int(table["obs"]["octave"][o])
    new_pose = []
    for q in range(Q):
        Siw = corrected[q]
        R = quat_to_R(Siw[0])[0]
        t = Siw[1][0] * (1. / Siw[2][0])
        T = np.eye(4, dtype=F32)
        T[:3, :3] = R.astype(F32)
        T[:3, 3] = t.astype(F32)
        new_pose.append((T, set_pose(T)[0]))
        out["Tiw_new"][q], out["Ow_new"][q] = new_pose[q]
    if mutation == "all_observers_corrected":
        for q in range(Q):
            Ow[qk[q]] = new_pose[q][1]
    names = {}      # point -> the positions that name it (for the ownership mutation only)
    for q in range(Q):
        for p in queries["feat"]["point"][queries["feat_off"][q]:queries["feat_off"][q + 1]]:
            names.setdefault(int(p), []).append(q)
    corrected_by_cur = np.zeros(P, bool)      # mnCorrectedByKF == mpCurrentKF->mnId
    for q in range(Q):
        Swi = inverse(corrected[q])
        Siw = non_corrected[q]
        for p in queries["feat"]["point"][queries["feat_off"][q]:queries["feat_off"][q + 1]]:
            p = int(p)
            if p < 0:
                continue
            if table["pts"]["bad"][p]:
                continue
            if corrected_by_cur[p]:
                continue
            if mutation == "last_keyframe_owns" and q != names[p][-1]:
                continue
            P3Dw = table["pts"]["pos"][p].astype(F64)[None]
            if mutation == "maps_swapped":
                c = smap(Siw, smap(Swi, P3Dw))
            else:
                c = smap(Swi, smap(Siw, P3Dw))
            out["pos"][p] = c[0].astype(F32)
            corrected_by_cur[p] = True
            out["corrected_ref"][p] = qk[q]
            out["normals"][p] = update_normal(table, p, out["pos"][p], Ow, octave_of)
        if mutation not in ("no_observer_corrected", "all_observers_corrected"):
            Ow[qk[q]] = new_pose[q][1]      # :522
    return out


def spread_global_ba(sc, mutation=None):
    """sc: dict with Tcw, TcwGBA [K, 4, 4], kf_in_gba [K], children (K ascending lists), parent [K] (mpParent: read by a mutation only),
    origins, pos, posGBA [P, 3], pt_in_gba, ref_kf, bad [P] -> dict of SPREAD_ARRAYS + levels"""
    assert mutation is None or mutation in MUTATIONS
    K, P = len(sc["kf_in_gba"]), len(sc["bad"])
    pose = [np.ascontiguousarray(sc["Tcw"][k], F32).copy() for k in range(K)]
    gba = [np.ascontiguousarray(sc["TcwGBA"][k], F32).copy() for k in range(K)]
    mark = [bool(x) for x in sc["kf_in_gba"]]
    children = [sorted(int(c) for c in cs) for cs in sc["children"]]
    if mutation == "parent_pointers":
        children = [[c for c in range(K) if int(sc["parent"][c]) == k] for k in range(K)]
    bef, depth = {}, {}
    queue = [int(o) for o in sc["origins"]]
    for o in queue:
        depth[o] = 0
    while queue:
        k = queue[0]
        _, Twc = set_pose(gba[k] if mutation == "parent_new_pose" else pose[k])      # GetPoseInverse(), :692
        for c in children[k]:
            depth[c] = 0
            if not mark[c]:
                Tchildc = gemm44(pose[c], Twc)
                gba[c] = gemm44(Tchildc, gba[k])
                mark[c] = True
                depth[c] = depth[k] + 1
            queue.append(c)
        bef[k] = pose[k].copy()
        pose[k] = gba[k].copy()      # SetPose(mTcwGBA), :707
        queue.pop(0)
    out = {"Tcw_new": np.stack(pose) if K else np.zeros((0, 4, 4), F32), "TcwGBA": np.stack(gba) if K else np.zeros((0, 4, 4), F32),
           "kf_marked": np.array(mark, np.uint8), "kf_reached": np.array([k in bef for k in range(K)], np.uint8), "pos": np.ascontiguousarray(sc["pos"], F32).copy(), "status": np.zeros(P, np.int32),
           "levels": max(depth.values()) if depth else 0}
    for p in range(P):
        if sc["bad"][p]:
            continue
        if sc["pt_in_gba"][p]:
            out["pos"][p] = sc["posGBA"][p]
            out["status"][p] = SPREAD_GBA
            continue
        r = int(sc["ref_kf"][p])
        if r < 0:
            out["status"][p] = SPREAD_UNDEFINED      # a NULL pRefKF
            continue
        if not mark[r]:
            continue
        if r not in bef:
            out["status"][p] = SPREAD_UNDEFINED      # mTcwBefGBA is empty
            continue
        Xc = gemv3_add(bef[r][:3, :3], sc["pos"][p], bef[r][:3, 3])
        twc, Twc = set_pose(pose[r])
        out["pos"][p] = gemv3_add(Twc[:3, :3], Xc, twc)
        out["status"][p] = SPREAD_MOVED
    return out
