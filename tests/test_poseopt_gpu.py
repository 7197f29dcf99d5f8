"""GPU: k_pose_opt (orbo_pose_optimization*, csrc/orbx_poseopt.hip) against the numpy restatement tests/pose_ref.py, at the shapes of
tests/pose_scene.py: CASES.  Flags and counts equal; the float pose within 1 ulp; the double pose within 64 x the deviation the
restatement itself shows when its edges are summed in 16 random orders (the kernel differs from it by its summation order and by
the device's sqrt / sin / cos / division); two runs byte-identical; a batch equal to its single calls; the device form equal to the
host form, also from a second host thread after orbx_thread_release_scratch, and also past the LDS stage with octaves outside the
level table; a batch that outgrows the staging pair's floor equal to its single calls."""
import os
import re
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pose_ref as R        # noqa: E402
import pose_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
MARGIN = 1e-5       # |chi2 / threshold - 1| below which a flag may differ: two orders above the float rounding of chi2
_refs = {}


def reference(name):
    """the restatement's result for a case, and S: its largest deviation in t / q over 16 random edge orders.  Computed once."""
    if name not in _refs:
        sc = S.case(name)
        n = len(sc["obs"])
        mark = np.where(sc["obs"]["valid"] == 0, 5, 1).astype(np.uint8)      # invalid entries must keep the 5, valid ones lose the 1
        ref = R.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"], outlier=mark)
        rng = np.random.default_rng(1234)
        dev = 0.0
        for _ in range(16):
            o = R.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"], outlier=mark, order=rng.permutation(n))
            dev = max(dev, np.abs(o["t"] - ref["t"]).max(), np.abs(o["q"] - ref["q"]).max())
        _refs[name] = (sc, mark, ref, dev)
    return _refs[name]


def as_bytes(res):
    T, out, ng, info = res
    return (T.tobytes(), out.tobytes(), ng, info["correspondences"], info["bad"], info["rounds"], tuple(info["iterations"]),
            tuple(info["trials"]), info["t"].tobytes(), info["q"].tobytes())


def check_against_reference(name, res):
    sc, mark, ref, dev = reference(name)
    T, out, ng, info = res
    # the condition of the comparison: no edge of the scene within the margin of its threshold, in any round
    for r, tr in enumerate(ref["trace"]):
        assert tr["min_margin"] > MARGIN, "scene %s: an edge is %.2e from its threshold in round %d - choose another seed" % (name, tr["min_margin"], r)
    assert (ng, info["correspondences"], info["bad"], info["rounds"]) == (ref["ngood"], ref["correspondences"], ref["bad"], ref["rounds"])
    assert (out == ref["outlier"]).all()
    inv = sc["obs"]["valid"] == 0
    assert (out[inv] == 5).all() and (out[~inv] <= 1).all()
    ulp = np.spacing(np.maximum(np.float32(1), np.abs(ref["Tcw"])).astype(np.float32))
    assert (np.abs(T.astype(np.float64) - ref["Tcw"].astype(np.float64)) <= ulp).all(), (T, ref["Tcw"])
    diff = max(np.abs(info["t"] - ref["t"]).max(), np.abs(info["q"] - ref["q"]).max())
    print("%s: S = %.3e, kernel - restatement = %.3e, float pose equal: %s" % (name, dev, diff, (T == ref["Tcw"]).all()))
    print("%s: iterations %s / %s, trials %s / %s (kernel / restatement), min |rho| %s" % (
        name, info["iterations"], ref["iterations"], info["trials"], ref["trials"], ["%.1e" % t["min_abs_rho"] for t in ref["trace"]]))
    assert diff <= 64 * dev, (diff, dev)
    for r, tr in enumerate(ref["trace"]):
        if tr["min_abs_rho"] > 1e-6:      # at convergence the sign of rho is rounding noise, and either branch gives the same pose
            assert (info["iterations"][r], info["trials"][r]) == (ref["iterations"][r], ref["trials"][r]), r
    assert all(info["iterations"][r] == 0 and info["trials"][r] == 0 for r in range(ref["rounds"], 4))


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernel_against_restatement(pkg, name):
    sc, mark, ref, dev = reference(name)
    res = pkg.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"], outlier=mark)
    check_against_reference(name, res)
    again = pkg.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"], outlier=mark)
    assert as_bytes(res) == as_bytes(again)                                    # determinism: identical bytes in all outputs


def test_fewer_than_three_correspondences(pkg):
    for name in ("n0", "n2"):
        sc = S.case(name)
        n = len(sc["obs"])
        T, out, ng, info = pkg.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"], outlier=np.ones(n, np.uint8))
        assert ng == 0 and (T == sc["Tcw0"]).all() and (out == 0).all() and info["correspondences"] == n and info["rounds"] == 0
    # three entries, one of them without a map point: 2 correspondences, its flag stays
    sc = S.case("n3")
    obs = sc["obs"].copy(); obs["valid"][1] = 0
    T, out, ng, info = pkg.pose_optimization(obs, sc["cam"], sc["Tcw0"], outlier=np.array([1, 9, 1], np.uint8))
    assert ng == 0 and (T == sc["Tcw0"]).all() and list(out) == [0, 9, 0] and info["correspondences"] == 2


def test_rejected_trial_and_break_are_reached(pkg):
    """the branches the cases are there for, read from the library's own counts"""
    info = pkg.pose_optimization(S.case("far")["obs"], S.CAM, S.case("far")["Tcw0"])[3]
    assert max(t - i for t, i in zip(info["trials"], info["iterations"])) > 0          # more solves than iterations: a rejected trial
    assert pkg.pose_optimization(S.case("n9")["obs"], S.CAM, S.case("n9")["Tcw0"])[3]["rounds"] == 1
    assert pkg.pose_optimization(S.case("n10")["obs"], S.CAM, S.case("n10")["Tcw0"])[3]["rounds"] == 4


def lds_edges():
    """PO_LDS_EDGES of csrc/orbx_poseopt.hip: the edges the kernel stages in LDS"""
    txt = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "orb_slam2v2-1_amd", "csrc", "orbx_poseopt.hip")).read()
    return int(re.search(r"^#define\s+PO_LDS_EDGES\s+(\d+)\b", txt, flags=re.M).group(1))


def test_edges_behind_the_lds_stage(pkg):
    """more edges than the kernel stages in LDS (1536): the rest is read from memory, same arithmetic"""
    assert (S.CASES["n1536"]["n"], S.CASES["n1537"]["n"]) == (lds_edges(), lds_edges() + 1) and S.CASES["n2000"]["n"] == 2000 > lds_edges()
    sc = S.case("n2000")
    ref = R.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"])
    T, out, ng, info = pkg.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"])
    assert min(t["min_margin"] for t in ref["trace"]) > MARGIN
    assert ng == ref["ngood"] and (out == ref["outlier"]).all() and info["rounds"] == 4
    ulp = np.spacing(np.maximum(np.float32(1), np.abs(ref["Tcw"])).astype(np.float32))
    assert (np.abs(T.astype(np.float64) - ref["Tcw"].astype(np.float64)) <= ulp).all()
    # and the full comparison: the double pose, the iteration and trial counts, the markers of the invalid entries
    check_against_reference("n2000", pkg.pose_optimization(sc["obs"], sc["cam"], sc["Tcw0"], outlier=reference("n2000")[1]))


def device_arrays(pkg, name, low, high):
    """the Frame arrays of a scene as the device form reads them - keypoint records, uright, world positions - with octave -1 at
    `low` and octave nlevels at `high`, and the host-form observations of the same call: inv_sigma2 of level 0 and of level
    nlevels - 1 there, which is the kernel's clamp as written (Frame produces neither octave)"""
    sc = S.case(name)
    obs, n = sc["obs"].copy(), len(sc["obs"])
    octave = sc["octave"].astype(np.int32)
    assert (obs["inv_sigma2"] == S.INV_SIGMA2[octave]).all()
    octave[low], octave[high] = -1, S.NLEVELS
    obs["inv_sigma2"] = S.INV_SIGMA2[np.clip(octave, 0, S.NLEVELS - 1)]
    kp = np.zeros(n, pkg.KP_DTYPE)
    kp["x"], kp["y"], kp["size"], kp["angle"], kp["response"], kp["octave"], kp["class_id"] = obs["u"], obs["v"], 31.0, 45.0, 20.0, octave, -1
    pts = np.zeros(n, pkg.POSE_WORLDPOS_DTYPE)
    for a in ("valid", "wx", "wy", "wz"):
        pts[a] = obs[a]
    return sc, obs, kp, np.ascontiguousarray(obs["ur"], np.float32), pts


@pytest.mark.parametrize("name", ["n1537", "n2000"])
def test_device_form_past_the_lds_stage(pkg, name):
    """The device form's fetch - keypoint record, uright, world position, the clamped octave - on both sides of the LDS stage: equal
    to the host form on the same observations, bit for bit.  n1537 has ONE edge past the stage, which takes octave nlevels (the
    clamp that would otherwise read past the level table); n2000 has half of each handful past it."""
    import torch
    E = lds_edges()
    valid = np.nonzero(S.case(name)["obs"]["valid"])[0]
    below, past = valid[valid < E], valid[valid >= E]
    if name == "n1537":
        assert list(past) == [E]                                           # the one edge read from memory is a correspondence
        low, high = below[[3, 700, 1400]], np.concatenate([below[[5, 900]], past])
    else:
        low, high = np.concatenate([below[[3, 1400]], past[[0, 200]]]), np.concatenate([below[[5, 900]], past[[1, -1]]])
    assert (low >= E).sum() * 2 in (0, len(low)) and (high >= E).any() and not set(low) & set(high)
    sc, obs, kp, ur, pts = device_arrays(pkg, name, low, high)
    assert len({float(obs["inv_sigma2"][i]) for i in high}) == 1 and obs["inv_sigma2"][low[0]] == 1.0
    assert (obs["inv_sigma2"] != sc["obs"]["inv_sigma2"]).sum() >= 2       # the clamped levels are not the scene's own
    mark = np.where(obs["valid"] == 0, 5, 1).astype(np.uint8)
    host = pkg.pose_optimization(obs, sc["cam"], sc["Tcw0"], outlier=mark)
    d_kp, d_ur = torch.from_numpy(kp.view(np.uint8).copy()).cuda(), torch.from_numpy(ur.copy()).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    torch.cuda.synchronize()
    dev = pkg.pose_optimization_device(d_kp.data_ptr(), d_ur.data_ptr(), len(obs), S.INV_SIGMA2, pts, sc["cam"], sc["Tcw0"], outlier=mark,
                                       stream=stream)
    assert as_bytes(dev) == as_bytes(host)
    inv = obs["valid"] == 0
    assert inv.any() and (host[1][inv] == 5).all() and (host[1][~inv] <= 1).all() and host[3]["rounds"] == 4
    assert host[2] > 0.6 * (~inv).sum()                                    # and the pose is one that explains the inliers


def test_batch_past_the_stage_and_the_floor(pkg):
    """[n65, n1537 x K, n2, n1536] in one launch from a fresh host thread, after n65 alone reserved the staging pair at its 256 KiB
    floor: the observations alone exceed the floor, so the pair regrows; the LDS is sized for the largest problem while the small
    ones stage only their own edges; flags and chi2 sit at offsets up to K x 1537.  Every problem equals its single call."""
    n_big = S.CASES["n1537"]["n"]
    K = (1 << 18) // (32 * n_big) + 1                               # the smallest K with K x 1537 observations > 256 KiB
    assert pkg.POSE_OBS_DTYPE.itemsize == 32 and (K - 1) * 32 * n_big <= 1 << 18 < K * 32 * n_big
    names = ["n65"] + ["n1537"] * K + ["n2", "n1536"]
    scs = {n: (S.case(n), np.where(S.case(n)["obs"]["valid"] == 0, 5, 1).astype(np.uint8)) for n in set(names)}
    obs = np.concatenate([scs[n][0]["obs"] for n in names])
    mark = np.concatenate([scs[n][1] for n in names])
    off = np.cumsum([0] + [len(scs[n][0]["obs"]) for n in names])
    single = lambda n: pkg.pose_optimization(scs[n][0]["obs"], S.CAM, scs[n][0]["Tcw0"], outlier=scs[n][1])      # noqa: E731
    got = {}

    def worker():
        try:
            got["first"] = as_bytes(single("n65"))
            got["batch"] = pkg.pose_optimization_batch(obs, off, [S.CAM] * len(names), [scs[n][0]["Tcw0"] for n in names], outlier=mark)
            got["again"] = as_bytes(single("n65"))
            got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001
            got["error"] = e

    th = threading.Thread(target=worker)
    th.start(); th.join()
    assert "error" not in got, got.get("error")
    one = {n: as_bytes(single(n)) for n in scs}
    Ts, out, ng, infos = got["batch"]
    for b, n in enumerate(names):
        assert as_bytes((Ts[b], out[off[b]:off[b + 1]], int(ng[b]), infos[b])) == one[n], (b, n)
    assert got["first"] == got["again"] == one["n65"] and got["rc"] == pkg.ORBX_OK


def test_batch_equals_single_calls(pkg):
    names = ("n2", "n65", "mixed300")
    scs = [S.case(n) for n in names]
    obs = np.concatenate([s["obs"] for s in scs])
    off = np.cumsum([0] + [len(s["obs"]) for s in scs])
    assert list(np.diff(off)) == [2, 65, 300]
    mark = np.where(obs["valid"] == 0, 5, 1).astype(np.uint8)
    cams = [(S.FX, S.FY, S.CX, S.CY, S.BF, S.BF / S.FX), (S.FX * 1.01, S.FY, S.CX, S.CY + 2, S.BF, S.BF / S.FX), S.CAM]     # a camera per problem
    Ts, out, ng, infos = pkg.pose_optimization_batch(obs, off, cams, [s["Tcw0"] for s in scs], outlier=mark)
    for b, s in enumerate(scs):
        one = pkg.pose_optimization(s["obs"], cams[b], s["Tcw0"], outlier=mark[off[b]:off[b + 1]])
        assert as_bytes(one) == as_bytes((Ts[b], out[off[b]:off[b + 1]], int(ng[b]), infos[b])), names[b]
    check_against_reference("mixed300", (Ts[2], out[off[2]:], int(ng[2]), infos[2]))
    # an empty problem in the middle, and B = 0
    Ts, out, ng, infos = pkg.pose_optimization_batch(scs[1]["obs"], [0, 0, 65], [S.CAM] * 2, [scs[0]["Tcw0"], scs[1]["Tcw0"]])
    assert ng[0] == 0 and (Ts[0] == scs[0]["Tcw0"]).all() and ng[1] == reference("n65")[2]["ngood"]
    assert len(pkg.pose_optimization_batch(obs[:0], [0], [], np.zeros((0, 4, 4)))[2]) == 0


def test_device_form_equals_host_form(pkg, synth):
    """One synthetic stereo frame stays in HBM (orbx_stereo_frame_view); SearchByProjection(cur, last) on it against itself as the last
    frame; then the pose from the device arrays equals the pose from the downloaded arrays, bit for bit - also from a second host
    thread that released its scratch in between."""
    import torch
    w, h = 752, 480
    left, right = synth.stereo_pair_blocky(w, h, 7)
    ex = pkg.ORBextractor(1000, S.SCALE, S.NLEVELS, 20, 7)
    cam = pkg.Camera(*S.CAM)
    stream = torch.cuda.current_stream().cuda_stream
    f = ex.stereo_frame_view(left, right, S.BF, float(np.float32(S.BF) / np.float32(S.FX)))
    k, ur, depth, v = f["kl"].copy(), f["uright"].copy(), f["depth"].copy(), f["view"]
    n = len(k)
    # the last frame's map points: Frame::UnprojectStereo at the identity pose (src/Frame.cc:681-694)
    last = np.zeros(n, pkg.LASTPT_DTYPE)
    good = depth > 0
    fx, fy, cx, cy = (np.float32(c) for c in S.CAM[:4])
    last["has_mp"] = good
    last["wx"] = np.where(good, (k["x"] - cx) * depth / fx, 0)
    last["wy"] = np.where(good, (k["y"] - cy) * depth / fy, 0)
    last["wz"] = np.where(good, depth, 0)
    last["observations"], last["octave"], last["angle"] = 2, k["octave"], k["angle"]
    I = np.eye(4, dtype=np.float32)
    nm, cur = pkg.search_by_projection_frame_device(v.d_kl, v.d_dl, v.d_uright, n, pkg.grid_geom(w, h), ex.GetScaleFactors(), cam, I, I, last,
                                                    v.d_dl, np.full(n, -1, np.int32), None, 7.0, False, True, 0, stream)
    assert nm > 100, nm
    pts = np.zeros(n, pkg.POSE_WORLDPOS_DTYPE)
    m = cur >= 0
    pts["valid"] = m
    for a in ("wx", "wy", "wz"):
        pts[a][m] = last[a][cur[m]]
    is2 = np.asarray(ex.GetInverseScaleSigmaSquares(), np.float32)          # mvInvLevelSigma2
    guess = (S.pose([0.004, -0.006, 0.003], [0.05, -0.03, 0.08]) @ np.eye(4)).astype(np.float32)
    obs = np.zeros(n, pkg.POSE_OBS_DTYPE)
    obs["valid"], obs["u"], obs["v"], obs["ur"], obs["inv_sigma2"] = pts["valid"], k["x"], k["y"], ur, is2[k["octave"]]
    obs["wx"], obs["wy"], obs["wz"] = pts["wx"], pts["wy"], pts["wz"]
    mark = np.where(m, 1, 3).astype(np.uint8)
    host = pkg.pose_optimization(obs, cam, guess, outlier=mark)
    dev = pkg.pose_optimization_device(v.d_kl, v.d_uright, n, is2, pts, cam, guess, outlier=mark, stream=stream)
    assert as_bytes(dev) == as_bytes(host)
    assert host[2] >= 0.9 * nm and (host[1][~m] == 3).all() and host[3]["rounds"] == 4
    assert np.abs(host[0] - I).max() < 0.02, host[0]          # every point was seen from the identity pose
    got = {}

    def second_thread():
        try:
            got["a"] = as_bytes(pkg.pose_optimization_device(v.d_kl, v.d_uright, n, is2, pts, cam, guess, outlier=mark, stream=stream))
            assert pkg.matcher_lib().orbx_thread_release_scratch() == 0
            got["b"] = as_bytes(pkg.pose_optimization_device(v.d_kl, v.d_uright, n, is2, pts, cam, guess, outlier=mark))
            got["c"] = as_bytes(pkg.pose_optimization(obs, cam, guess, outlier=mark))
            assert pkg.matcher_lib().orbx_thread_release_scratch() == 0
        except Exception as e:      # noqa: BLE001
            got["error"] = e

    th = threading.Thread(target=second_thread)
    th.start(); th.join()
    assert "error" not in got, got.get("error")
    assert got["a"] == got["b"] == got["c"] == as_bytes(host)
    ex.close()
