"""GPU: LocalMapping's device steps chained on real features: two synthetic keyframes (a band scene seen by a camera and by one 11 cm
to its right) through the device extractor, the vocabulary descent, the chain orbl_create_new_map_points (ComputeF12, the baseline rule,
SearchForTriangulation, the triangulation and its tests), and the new points fed to orbm_best_in_windows as ORBmatcher::Fuse does.
Every step is fed with what the step before gave ON THE DEVICE and compared with its CPU counterpart on the same inputs: the oracle for
the extractor, the descent and the window search, tests/newpoints_ref.py for the chain.  The second camera stands exactly sideways, so
the epipole is not finite (-inf, NaN), as in the reference on such a pair: the matcher's epipole test then rejects nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bow_scene as bs           # noqa: E402
import newpoints_ref as R        # noqa: E402

pytestmark = pytest.mark.gpu
W, H, NF = 640, 480, 1000
FX, MBF = 435.2, 47.9
K = (FX, FX, W / 2, H / 2)
F32 = np.float32


@pytest.mark.parametrize("levelsup", [2, 3])      # 10 shared vocabulary nodes; one node that holds all 1004 candidates
def test_extract_bow_new_points_fuse(pkg, oracle, synth, levelsup):
    left, right = synth.stereo_pair_blocky(W, H, 42)
    # 1. the extractor
    kps, descs = [], []
    for img in (left, right):
        k, d = pkg.ORBextractor(NF, 1.2, 8, 20, 7, device=0)(img)
        ok_, od = oracle.Extractor(NF, 1.2, 8, 20, 7).extract(img)
        assert len(k) == len(ok_) and (d == od).all()
        for f in ("x", "y", "octave"):
            assert (k[f] == ok_[f]).all(), f
        kps.append(k); descs.append(d)
    (k1, k2), (d1, d2) = kps, descs
    # 2. the vocabulary descent: the feature vectors of both keyframes
    voc = bs.make_vocabulary(np.random.default_rng(5))
    gv = pkg.Vocabulary(voc["k"], voc["L"], 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    ov = oracle.Vocabulary(voc["k"], voc["L"], 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    fvs = []
    for d in (d1, d2):
        _, nid, wt = gv.transform(d, levelsup)
        fv = {}
        for i, n in enumerate(nid):
            if wt[i] > 0:                       # a stopped word adds nothing to either vector (DBoW2's transform)
                fv.setdefault(int(n), []).append(i)
        assert fv == ov.transform(d, levelsup)[2]
        fvs.append(fv)
    nqs, qi, ncs, ci = bs.intersect(fvs[0], fvs[1])
    # 3. CreateNewMapPoints: the views, F12, the epipole as ORBmatcher forms it, then the chain
    sf = np.array([1.2 ** l for l in range(8)], F32)
    sig2 = sf * sf
    b = float(F32(MBF) / F32(FX))
    T1, T2 = np.eye(4, dtype=F32), np.eye(4, dtype=F32)
    T2[0, 3] = -b
    v1, v2 = pkg.newpoints_view(T1, K, b, MBF, 1.2, 8), pkg.newpoints_view(T2, K, b, MBF, 1.2, 8)
    assert v2.tobytes() == R.view(T2, K, b, MBF, 1.2, 8).tobytes()
    F12 = pkg.compute_f12(T1, K, T2, K)
    assert F12.tobytes() == R.compute_f12(T1, K, T2, K).tobytes()
    Cc = R._mv(T2[:3, :3], v1["Ow"].reshape(1, 3), T2[:3, 3]).reshape(3)
    with np.errstate(all="ignore"):
        invz = F32(1.0) / Cc[2]
        ex, ey = F32(K[0]) * Cc[0] * invz + F32(K[2]), F32(K[1]) * Cc[1] * invz + F32(K[3])
    assert not np.isfinite(ex) and np.isnan(ey)
    flags1, flags2 = np.ones(len(k1), np.uint8), np.ones(len(k2), np.uint8)
    cur, nbk = {"view": v1, "kp": k1, "st": None, "sf": sf, "sig2": sig2}, {"view": v2, "kp": k2, "st": None, "sf": sf, "sig2": sig2}
    nb = {"kf": nbk, "cd": d2, "cf": flags2, "nqs": nqs, "qi": qi, "ncs": ncs, "ci": ci, "F12": F12, "ex": ex, "ey": ey, "median": F32(2.0)}
    ref = R.create_new_map_points(cur, d1, flags1, [nb], True)
    gcur = pkg.newpoints_keyframe(v1, k1, None, sf, sig2)
    gnb = pkg.newpoints_neighbour(pkg.newpoints_keyframe(v2, k2, None, sf, sig2), d2, flags2, nqs, qi, ncs, ci, F12, ex, ey, 2.0)
    got = pkg.create_new_map_points(gcur, d1, flags1, [gnb], True)
    for f in ("match_q", "nmatches", "nnew", "skipped", "q_flags"):
        assert (got[f] == ref[f]).all(), f
    assert got["points"].tobytes() == ref["points"].tobytes()        # monocular: no device transcendental on the path
    new = np.flatnonzero(got["points"]["status"][0] >= 0)
    print("levelsup %d: %d shared nodes, %d matches, %d new points" % (levelsup, len(nqs) - 1, got["nmatches"][0], len(new)))
    assert len(new) >= 20 and not got["skipped"][0]
    # the points are where the bands are: depth = fx b / disparity, disparities of 2 .. 60 px
    idx2 = got["match_q"][0][new]
    disp = k1["x"][new] - k2["x"][idx2]
    assert np.abs(got["points"]["z"][0][new] - MBF / disp).max() < 0.05 * (MBF / disp).max()
    # 4. Fuse: the new points projected into keyframe 2 find the very features they were triangulated from
    P = got["points"][0][new]
    X = np.stack([P["x"], P["y"], P["z"]], axis=1).astype(np.float64)
    pts = np.zeros(len(new), oracle.MP3D_DTYPE)
    pts["valid"], pts["wx"], pts["wy"], pts["wz"] = 1, P["x"], P["y"], P["z"]
    n1, n2 = X - v1["Ow"], X - v2["Ow"]
    nrm = 0.5 * (n1 / np.linalg.norm(n1, axis=1)[:, None] + n2 / np.linalg.norm(n2, axis=1)[:, None])      # UpdateNormalAndDepth
    pts["nx"], pts["ny"], pts["nz"] = nrm[:, 0], nrm[:, 1], nrm[:, 2]
    pts["max_distance"] = np.linalg.norm(n1, axis=1) * sf[k1["octave"][new]]
    pts["min_distance"] = pts["max_distance"] / sf[7]
    ocam, og, pg = oracle.Cam(FX, FX, W / 2, H / 2, MBF, b), oracle.grid_geom(W, H), pkg.grid_geom(W, H)
    q = oracle.pose_window_queries(pts, og, sf, float(np.log(F32(1.2))), ocam, T2, 3.0)
    inv_s2 = (1.0 / sig2).astype(F32)
    obi, obd = oracle.best_in_windows(k2, d2, None, og, q, d1[new], inv_s2)
    gbi, gbd = pkg.best_in_windows(k2, d2, None, pg, q, d1[new], inv_s2)
    assert (gbi == obi).all() and (gbd == obd).all()
    assert (gbi == idx2).sum() >= 0.8 * len(new), ((gbi == idx2).sum(), len(new))
