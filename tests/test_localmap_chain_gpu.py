"""GPU: Tracking::TrackLocalMap end to end on a small synthetic map: a dozen keyframes on a path, a frame whose keypoints sit at the
projections of map points with descriptors a few bits off.  LocalMap.update -> search_local_points -> pose_optimization, each stage fed
with the outputs of the one before.  The integer stages are byte-equal to the CPU chain (the restatement tests/localmap_ref.py, the C
oracle's isInFrustum + SearchByProjection, tests/pose_ref.py), and the pose is checked by test_poseopt_gpu.check_against_reference's
existing rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_ref as LR        # noqa: E402
import pose_ref                  # noqa: E402
import test_poseopt_gpu as TP    # noqa: E402
from test_localmap_gpu import assert_same, frame_scene, run_frame, set_scene      # noqa: E402

pytestmark = pytest.mark.gpu
NAME = "localmap_chain"


def observations(fr, sc, frame_points):
    """Optimizer::PoseOptimization's edges from the frame's slots: the keypoint, its level's sigma and the point's position"""
    k, sf = fr["k"], fr["sf"]
    has = frame_points >= 0
    pos = sc["table"]["pts"]["pos"][np.maximum(frame_points, 0)]
    obs = np.zeros(len(k), pose_ref.OBS_DTYPE)
    inv_sigma2 = (np.float32(1) / (sf * sf)).astype(np.float32)
    obs["valid"], obs["u"], obs["v"], obs["ur"], obs["inv_sigma2"] = has, k["x"], k["y"], fr["uright"], inv_sigma2[k["octave"]]
    for j, a in enumerate(("wx", "wy", "wz")):
        obs[a] = np.where(has, pos[:, j], 0)
    return obs


def slots_after_search(frame_points, local_pts, frame_mp):
    """mCurrentFrame.mvpMapPoints after SearchByProjection: a local index names its point, -2 keeps the point the slot held"""
    return np.where(frame_mp >= 0, local_pts[np.maximum(frame_mp, 0)] if len(local_pts) else -1, np.where(frame_mp == -2, frame_points, -1)).astype(np.int32)


def test_track_local_map_chain(pkg, oracle, synth):
    sc, fr = frame_scene(pkg, oracle, synth, K=12)
    k, d, uright, w, h, sf, T = fr["k"], fr["d"], fr["uright"], fr["w"], fr["h"], fr["sf"], fr["T"]
    cam6 = (fr["fx"], fr["fy"], fr["cx"], fr["cy"], fr["mbf"], np.float32(fr["mbf"]) / np.float32(fr["fx"]))
    # ---- the CPU chain
    want = LR.update_local_map(sc)
    ocam = fr["oracle_cam"]
    proj = oracle.is_in_frustum(want["pts"][list(oracle.MP3D_DTYPE.names)], want["pts"]["observations"], T, ocam, oracle.grid_geom(w, h), 0.5, fr["log_sf"], 8)
    on, ofm = oracle.search_by_projection_mp(k, d, uright, oracle.grid_geom(w, h), sf, proj, want["mp_desc"], want["holder"], want["ext_obs"], 1.0, 0.8)
    wslots = slots_after_search(want["frame_points"], want["local_pts"], ofm)
    wobs = observations(fr, sc, wslots)
    Tcw0 = T.copy()
    Tcw0[:3, 3] += np.array([0.02, -0.01, 0.03], np.float32)
    mark = np.where(wobs["valid"] == 0, 5, 1).astype(np.uint8)
    if NAME not in TP._refs:
        ref = pose_ref.pose_optimization(wobs, cam6, Tcw0, outlier=mark)
        rng, dev = np.random.default_rng(1234), 0.0
        for _ in range(16):
            o = pose_ref.pose_optimization(wobs, cam6, Tcw0, outlier=mark, order=rng.permutation(len(wobs)))
            dev = max(dev, np.abs(o["t"] - ref["t"]).max(), np.abs(o["q"] - ref["q"]).max())
        TP._refs[NAME] = ({"obs": wobs, "cam": cam6, "Tcw0": Tcw0}, mark, ref, dev)
    assert len(want["local_kf"]) == 12 and on > 100 and TP._refs[NAME][2]["ngood"] > 100
    # ---- the device chain
    with pkg.LocalMap() as lm:
        set_scene(lm, sc)
        out = run_frame(lm, sc)
    assert_same(out, want)
    thr = pkg.predict_scale_thresholds(fr["log_sf"], 8)
    gn, gfm, gproj = pkg.search_local_points(k, d, uright, pkg.grid_geom(w, h), sf, out["pts"], out["mp_desc"], T, pkg.Camera(*cam6), 0.5, thr, out["holder"],
                                             out["ext_obs"], 1.0, 0.8)
    assert gn == on and gfm.tobytes() == ofm.tobytes() and gproj.tobytes() == proj.tobytes()
    gslots = slots_after_search(out["frame_points"], out["local_pts"], gfm)
    gobs = observations(fr, sc, gslots)
    assert gslots.tobytes() == wslots.tobytes() and gobs.tobytes() == wobs.tobytes()
    TP.check_against_reference(NAME, pkg.pose_optimization(gobs, cam6, Tcw0, outlier=mark))
