"""GPU: the local map through LocalMap on every scene of tests/localmap_scene.py.  Every output byte equals the literal restatement
tests/localmap_ref.py; two different frames one after the other on one handle equal their fresh-handle results (the cleaning pass); the
same frame twice gives the same bytes; a larger and then a smaller map on one handle (regrow); and the outputs fed unchanged to
search_local_points give the matches of the arrays packed the old way from the restatement's lists."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_ref as LR        # noqa: E402
import localmap_scene as S       # noqa: E402
from test_localmap_cpu import graph_of      # noqa: E402

pytestmark = pytest.mark.gpu


def set_scene(lm, sc):
    lm.set_map(sc["table"], sc["features"], graph_of(None, sc), sc["views"], sc["desc"])


def run_frame(lm, sc):
    return lm.update(sc["frame_points"], sc["prev_kf"], max_keyframes=sc["max_keyframes"], nbest=sc["nbest"])


def got_bytes(out):
    return [np.array([out["info"][k] for k in LR.INFO_FIELDS], np.int32).tobytes()] + [np.ascontiguousarray(out[k]).tobytes() for k in LR.ARRAYS]


def assert_same(out, want):
    for k in LR.ARRAYS:
        assert out[k].dtype == want[k].dtype and out[k].shape == want[k].shape, k
    assert got_bytes(out) == LR.result_bytes(want)
    assert out["info"]["launches"] == 8 and 1 <= out["info"]["syncs"] <= 2


def other_frame(sc, seed):
    """another frame over the same map: other points, other previous keyframes"""
    rng = np.random.default_rng(seed)
    P, K = len(sc["table"]["pts"]), len(sc["table"]["kf"])
    fr = rng.integers(-1, P, 300).astype(np.int32)
    return dict(sc, frame_points=fr, prev_kf=rng.choice(K, 4, replace=False).astype(np.int32), max_keyframes=12)


@pytest.mark.parametrize("name", list(S.SCENES))
def test_every_scene_equals_the_restatement(pkg, name):
    sc = S.scene(name)
    with pkg.LocalMap() as lm:
        set_scene(lm, sc)
        assert_same(run_frame(lm, sc), S.expected(name))


def test_frames_in_a_row_on_one_handle(pkg):
    """the state a frame leaves is idle: frame A, frame B, an empty-vote frame and A again on one handle equal the restatement, which
    starts every frame from fresh objects"""
    a = S.scene("random")
    b, c = other_frame(a, 5), dict(a, frame_points=np.full(7, -1, np.int32))
    wa, wb, wc = S.expected("random"), LR.update_local_map(b), LR.update_local_map(c)
    assert wc["info"]["empty_vote"] == 1 and len(wb["local_pts"]) > 100 and wb["local_pts"].tobytes() != wa["local_pts"].tobytes()
    with pkg.LocalMap() as lm:
        set_scene(lm, a)
        for sc, want in ((a, wa), (b, wb), (c, wc), (a, wa), (a, wa)):
            assert_same(run_frame(lm, sc), want)


def test_larger_then_smaller_map_on_one_handle(pkg):
    small, big, mid = S.scene("plain"), S.scene("random"), S.scene("m_257")
    with pkg.LocalMap() as lm:
        for name, sc in (("plain", small), ("random", big), ("m_257", mid), ("plain", small), ("K_lds_plus_1", S.scene("K_lds_plus_1")), ("random", big)):
            set_scene(lm, sc)
            assert_same(run_frame(lm, sc), S.expected(name))
        i = lm.info()
        assert (i["K"], i["P"]) == (60, 3000) and i["device_bytes"] >= i["snapshot_bytes"] > 0


def pack_the_old_way(sc, local_pts, fp):
    """what SearchLocalPointsHIP (host/ORBmatcher.cc) builds from mvpLocalMapPoints and the frame's slots"""
    m = len(local_pts)
    wp, pd = np.zeros(m, LR.WORLDPOINT_DTYPE), np.zeros((m, 32), np.uint8)
    seen = set(int(p) for p in fp if p >= 0)
    index = {}
    for j, p in enumerate(local_pts):
        p = int(p)
        index[p] = j
        wp["observations"][j] = sc["views"]["observations"][p]
        if p in seen or sc["table"]["pts"]["bad"][p]:
            continue
        wp["valid"][j] = 1
        wp["wx"][j], wp["wy"][j], wp["wz"][j] = sc["table"]["pts"]["pos"][p]
        wp["nx"][j], wp["ny"][j], wp["nz"][j] = sc["views"]["normal"][p]
        wp["max_distance"][j], wp["min_distance"][j] = sc["views"]["max_distance"][p], sc["views"]["min_distance"][p]
        pd[j] = sc["desc"][p]
    holder, ext = np.full(len(fp), -1, np.int32), np.zeros(len(fp), np.int32)
    for i, p in enumerate(fp):
        if p >= 0:
            if int(p) in index:
                holder[i] = index[int(p)]
            else:
                holder[i], ext[i] = -2, sc["views"]["observations"][int(p)]
    return wp, pd, holder, ext


def frame_scene(pkg, oracle, synth, K=6):
    """a frame of real keypoints over a map of 600 world points that project into it, K keyframes on a path
    -> (scene, dict of the frame: k, d, uright, geometry, pose, camera)"""
    import covis_ref as R
    import match_cases as mc
    ks, w, h, rng, k, d, sf, cam, log_sf, T, pts3, wp0, pd0, obs = mc.local_map(pkg, oracle, synth, 7, m=600)
    P, n = len(wp0), len(k)
    kf = np.zeros(K, R.KEYFRAME_DTYPE)
    kf["id"] = np.arange(K)
    pts = np.zeros(P, R.POINT_DTYPE)
    pts["pos"] = np.stack([wp0["wx"], wp0["wy"], wp0["wz"]], 1)
    pts["ref_kf"] = -1
    pts["bad"][rng.choice(P, 20, replace=False)] = 1
    kf_points = [[int(p) for p in rng.choice(P, 180, replace=False)] for _ in range(K)]
    rows = [(p, s, i, 0, 0) for s, f in enumerate(kf_points) for i, p in enumerate(f)]
    feats = []
    for f in kf_points:
        a = np.zeros(len(f), R.FEATURE_DTYPE)
        a["point"] = f
        feats.append(a)
    views = np.zeros(P, LR.VIEW_DTYPE)
    views["normal"] = np.stack([wp0["nx"], wp0["ny"], wp0["nz"]], 1)
    views["max_distance"], views["min_distance"], views["observations"] = wp0["max_distance"], wp0["min_distance"], obs
    fp = np.full(n, -1, np.int32)
    held = rng.choice(n, 150, replace=False)
    fp[held] = rng.choice(P, 150, replace=False)
    sc = {"table": R.build_table(kf, pts, rows, sf), "features": R.build_queries(np.arange(K), feats), "parent": np.arange(-1, K - 1, dtype=np.int32),
          "cov": [[(s + 1) % K] for s in range(K)], "children": [[s + 1] if s + 1 < K else [] for s in range(K)], "views": views, "desc": pd0,
          "frame_points": fp, "prev_kf": np.zeros(0, np.int32), "max_keyframes": 80, "nbest": 10}
    uright = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 40, n), -1).astype(np.float32)
    frame = {"k": k, "d": d, "uright": uright, "w": w, "h": h, "sf": sf, "log_sf": log_sf, "T": T, "fx": ks.FX, "fy": ks.FY, "cx": ks.CX, "cy": ks.CY, "mbf": ks.MBF, "oracle_cam": cam}
    return sc, frame


def test_outputs_feed_search_local_points_unchanged(pkg, oracle, synth):
    """update's arrays go to search_local_points as they are, and the matches equal those of the arrays packed the old way from the
    restatement's lists"""
    sc, fr = frame_scene(pkg, oracle, synth)
    k, d, uright, w, h, sf, T = fr["k"], fr["d"], fr["uright"], fr["w"], fr["h"], fr["sf"], fr["T"]
    want = LR.update_local_map(sc)
    with pkg.LocalMap() as lm:
        set_scene(lm, sc)
        out = run_frame(lm, sc)
    assert_same(out, want)
    assert len(out["local_pts"]) > 400 and (out["holder"] == -2).any() and (out["holder"] >= 0).sum() > 50
    thr = pkg.predict_scale_thresholds(fr["log_sf"], 8)
    pcam = pkg.Camera(fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["mbf"], np.float32(fr["mbf"]) / np.float32(fr["fx"]))
    new = pkg.search_local_points(k, d, uright, pkg.grid_geom(w, h), sf, out["pts"], out["mp_desc"], T, pcam, 0.5, thr, out["holder"], out["ext_obs"], 1.0, 0.8)
    owp, opd, oholder, oext = pack_the_old_way(sc, want["local_pts"], want["frame_points"])
    old = pkg.search_local_points(k, d, uright, pkg.grid_geom(w, h), sf, owp, opd, T, pcam, 0.5, thr, oholder, oext, 1.0, 0.8)
    assert new[0] == old[0] > 100
    assert new[1].tobytes() == old[1].tobytes() and new[2].tobytes() == old[2].tobytes()
