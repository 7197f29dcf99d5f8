"""GPU: Tracking::Track's main loop chained on the device (tests/track_chain.py) over the scenes of tests/track_scene.py, stereo and
monocular: extraction -> SearchByProjection(cur, last) at a motion-model guess -> PoseOptimization -> SearchLocalPoints at the
optimised pose -> PoseOptimization -> the velocity from two estimated poses; monocular: SearchForInitialization -> Initialize ->
ComputeDistinctiveDescriptors -> the same loop with monocular edges.  Each stage is fed with what the stage before it gave ON THE
DEVICE; nothing is planted after the first stereo pose.  Two device backends: the host-array entry points, and the frame left in HBM
with the *_device matchers, pose_optimization_device and initialize_device reading it there.

Demand 1, stage by stage: every trace entry of a device chain is re-run through that stage's restatement on the inputs the device
chain gave it and held to the stage's own rule - extraction, stereo matches, the matchers, isInFrustum and the distinctive
descriptors byte-equal to the oracle; the Initializer by tests/test_initializer_gpu.py's rule (everything byte-equal, the parallax
within 4 ulp); the pose optimisation by test_poseopt_gpu.check_against_reference's rule (flags and counts equal, the float pose
within 1 ulp, iterations and trials equal where min |rho| > 1e-6).  An edge within MARGIN of its threshold on the device's inputs may
differ in its flag; such edges may be at most 0.5 % of the call's edges.  Restatements are memoised by input bytes.

Demand 2, end to end: the two device chains byte-identical in every trace entry; against the CPU chain every frame's trace equal up
to the first frame where a pose differs, that pose within 1 ulp; from there on Demand 1, every count rule of
track_scene.assert_counts, and the poses within 4 x the CPU chain's own error against the planted ones (track_scene.CPU_ERRORS,
measured on the CPU).  A second host thread, after orbx_thread_release_scratch, runs the stereo chain's last two frames from the
saved state and gets the same bytes.

On an MI355X both device chains of both scenes leave the CPU chain's bytes in every trace entry (no pose differs, no edge stands
within MARGIN); the four chains take 0.02 - 0.4 s each once the runtime is up."""
import hashlib
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_chain as K             # noqa: E402
import track_scene as S             # noqa: E402
from test_initializer_gpu import ulps                   # noqa: E402
from test_poseopt_gpu import MARGIN                     # noqa: E402
from test_reloc_chain_gpu import within_one_ulp         # noqa: E402

pytestmark = pytest.mark.gpu
BACKENDS = {"host": K.GpuHostBackend, "device": K.GpuDeviceBackend}
SAVE_AT = S.STEREO["T"] - 2
_runs = {}


def gpu_chain(mode, backend):
    """one device chain per scene and backend, shared by the tests"""
    if (mode, backend) not in _runs:
        _runs[(mode, backend)] = S.run(mode, BACKENDS[backend], **({"save_at": SAVE_AT} if mode == "stereo" else {}))
    return _runs[(mode, backend)]


def key(*parts):
    h = hashlib.sha1()
    for p in parts:
        h.update(np.ascontiguousarray(p).tobytes() if isinstance(p, np.ndarray) else repr(p).encode())
        h.update(b"|")
    return h.digest()


def check_optimize(where, i, o):
    """test_poseopt_gpu.check_against_reference's rule on a call of the chain"""
    r = K.restated_optimize(i["obs"], i["Tcw"], i["outlier"])
    info = o["info"]
    assert info["correspondences"] == r["correspondences"] and info["rounds"] == r["rounds"], where
    valid = i["obs"]["valid"] != 0
    assert (o["outlier"][~valid] == i["outlier"][~valid]).all() and (o["outlier"][valid] <= 1).all(), where      # stale flags stay
    if all(tr["min_margin"] > MARGIN for tr in r["trace"]):
        near = 0
        assert (o["ngood"], info["bad"]) == (r["ngood"], r["bad"]) and (o["outlier"] == r["outlier"]).all(), where
    else:                                   # an edge at its threshold on the device's own inputs: its flag may differ
        close = np.zeros(r["correspondences"], bool)
        for tr in r["trace"]:
            close |= tr["margins"] <= MARGIN
        near = int(close.sum())
        assert near <= 0.005 * r["correspondences"], (where, near)
        idx = np.nonzero(valid)[0]
        differ = o["outlier"] != r["outlier"]
        assert not differ[~valid].any() and not differ[idx[~close]].any(), where
        if differ.any():
            return near
    assert within_one_ulp(o["Tcw"], r["Tcw"]), (where, o["Tcw"], r["Tcw"])
    for rnd, tr in enumerate(r["trace"]):
        if tr["min_abs_rho"] > 1e-6:
            assert (info["iterations"][rnd], info["trials"][rnd]) == (r["iterations"][rnd], r["trials"][rnd]), (where, rnd)
    return near


def check_initialize(where, i, o):
    """tests/test_initializer_gpu.py: check_against_reference's rule, on the chain's own matches"""
    r = K.restated_initialize(i["keys1"], i["keys2"], i["matches"], i["sets"])
    S.assert_init_margins(r)
    info = o["info"]
    for k in ("SH", "SF", "RH"):
        assert np.float32(info[k]).tobytes() == np.float32(r[k]).tobytes(), (where, k)
    assert info["model"] == r["model"] and tuple(info["best_iteration"]) == tuple(r["best"]) and tuple(info["inliers"]) == r["inliers"], where
    assert info["H21"].tobytes() == r["H21"].tobytes() and info["F21"].tobytes() == r["F21"].tobytes(), where
    assert int(o["ok"]) == r["result"] and info["ncand"] == r["ncand"] and list(info["ngood"]) == r["ngood"], where
    assert (info["best_good"], info["second_good"]) == (r["best_good"], r["second_good"]), where
    assert o["R21"].tobytes() == r["R21"].tobytes() and o["t21"].tobytes() == r["t21"].tobytes() and o["P3D"].tobytes() == r["P3D"].tobytes(), where
    assert (o["triangulated"] == r["triangulated"]).all(), where
    assert ulps(info["parallax"], r["parallax"]) <= 4 and all(ulps(a, b) <= 4 for a, b in zip(info["cand_parallax"], r["cand_parallax"])), where
    if "search_call" in info:                                 # FindHomography / FindFundamental through orbi_search (the host-array backend)
        scores, iH, iF, sinfo = info["search_call"]
        s = r["search"]
        assert scores.tobytes() == s["scores"].tobytes() and (iH == s["inliersH"]).all() and (iF == s["inliersF"]).all(), where
        assert tuple(sinfo["best_iteration"]) == tuple(r["best"]) and sinfo["H21"].tobytes() == r["H21"].tobytes() and sinfo["F21"].tobytes() == r["F21"].tobytes()


def check_stages(mode, ch):
    """Demand 1 on a device chain's trace -> calls per stage, and the edges that stood within MARGIN of a threshold"""
    cpu = K.CpuBackend(S.W, S.H, 1000)
    ref_frames = {e["frame"]: e["out"] for e in S.cpu_chain(mode).trace if e["stage"] == "frame"}      # the oracle on the same images
    frames, n, near = {}, {}, 0
    for e in ch.trace:
        i, o, st, where = e["in"], e["out"], e["stage"], (mode, e["stage"], e["frame"])
        if st == "frame":
            frames[e["frame"]] = o
            for a, v in ref_frames[e["frame"]].items():
                assert o[a].tobytes() == v.tobytes(), (where, a)
        elif st == "project":
            f = dict(frames[e["frame"]], uright=frames[e["frame"]].get("uright", np.full(len(frames[e["frame"]]["k"]), -1.0, np.float32)))
            rn, rm = K.memo("project", key(f["k"], f["d"], f["uright"], i["Tcw"], i["last_Tcw"], i["last"], i["last_desc"], i["th"], i["mono"]),
                            lambda: cpu.search_frame(f, {"d": i["last_desc"]}, i["Tcw"], i["last_Tcw"], i["last"], np.full(len(f["k"]), -1, np.int32), i["th"], i["mono"]))
            assert o["n"] == rn and (o["match"] == rm).all(), where
        elif st == "local":
            f = dict(frames[e["frame"]], uright=frames[e["frame"]].get("uright", np.full(len(frames[e["frame"]]["k"]), -1.0, np.float32)))
            rn, rh, rp = K.memo("local", key(f["k"], f["d"], f["uright"], i["pts"], i["desc"], i["Tcw"], i["holder"], i["ext_obs"]),
                                lambda: cpu.search_local(f, i["pts"], i["desc"], i["Tcw"], i["holder"], i["ext_obs"], 1.0, 0.8, ch.log_sf))
            assert o["n"] == rn and (o["holder"] == rh).all() and o["frustum"].tobytes() == rp.tobytes(), where
        elif st.startswith("optimize"):
            near += check_optimize(where, i, o)
        elif st == "search_init":
            rn, rm, rp = cpu.search_init(frames[0], frames[1], i["prev"], 100)
            assert o["n"] == rn and (o["match"] == rm).all() and o["prev"].tobytes() == rp.tobytes(), where
        elif st == "initialize":
            check_initialize(where, i, o)
        elif st == "distinctive":
            assert (o["row"] == cpu.distinctive(i["desc"], i["offsets"])).all(), where
        else:
            continue                                     # host bookkeeping
        n[st] = n.get(st, 0) + 1
    return n, near


def frames_of(ch):
    out = {}
    for e in ch.trace:
        out.setdefault(e["frame"], []).append(K.entry_bytes(e))
    return out


def check_against_cpu(mode, ch):
    """Demand 2 against the CPU chain -> the first frame whose pose differs (None: none does)"""
    cpu = S.cpu_chain(mode)
    S.assert_counts(mode, ch)
    a, b = frames_of(ch), frames_of(cpu)
    assert sorted(a) == sorted(b)
    first = None
    for t in sorted(a):
        if a[t] == b[t]:
            continue
        ea, eb = [e for e in ch.trace if e["frame"] == t], [e for e in cpu.trace if e["frame"] == t]
        for x, y in zip(ea, eb):                         # the first entry that differs must be a pose within the 1-ulp rule
            if K.entry_bytes(x) != K.entry_bytes(y):
                assert x["stage"].startswith("optimize") and x["stage"] == y["stage"], (mode, t, x["stage"])
                assert (x["out"]["outlier"] == y["out"]["outlier"]).all() and x["out"]["ngood"] == y["out"]["ngood"], (mode, t)
                assert within_one_ulp(x["out"]["Tcw"], y["out"]["Tcw"]), (mode, t)
                break
        else:
            raise AssertionError((mode, t, "the frame's traces differ in length only", len(ea), len(eb)))
        first = t
        break
    ok, err = S.within_bounds(mode, ch)
    assert ok, (mode, err, S.CPU_ERRORS[mode])
    return first, err


@pytest.mark.parametrize("backend", list(BACKENDS))
@pytest.mark.parametrize("mode", ["stereo", "mono"])
def test_device_chain(mode, backend):
    ch = gpu_chain(mode, backend)
    assert ch.lost is None, ch.lost
    n, near = check_stages(mode, ch)
    first, err = check_against_cpu(mode, ch)
    assert (ch.inv_sigma2 == np.asarray(ch.be.exl.GetInverseScaleSigmaSquares(), np.float32)).all()      # mvInvLevelSigma2 as the chain indexes it
    expect = dict(frame=S.STEREO["T"], project=S.STEREO["T"] - 1, local=S.STEREO["T"] - 1, optimize_motion=S.STEREO["T"] - 1, optimize_local=S.STEREO["T"] - 1)
    if mode == "mono":
        expect = dict(frame=5, search_init=1, initialize=1, distinctive=1, project=3, local=3, optimize_motion=3, optimize_local=3)
    assert n == expect, n
    print("%s / %s: %.2f s; stage calls held to their restatements: %s; edges within MARGIN: %d; first frame whose pose differs from the CPU "
          "chain's: %s; errors against the planted poses %s; per frame %s" % (mode, backend, ch.seconds, n, near, first, err, ch.frames))


@pytest.mark.parametrize("mode", ["stereo", "mono"])
def test_host_and_device_forms_give_the_same_bytes(mode):
    a, b = gpu_chain(mode, "host"), gpu_chain(mode, "device")
    assert K.first_difference(a, b) is None, (mode, K.first_difference(a, b))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a.poses, b.poses)) and a.frames == b.frames
    if mode == "mono":
        assert a.init == b.init


def test_second_host_thread_continues_the_stereo_chain(pkg):
    """a second host thread builds its own extractor, scratch, mirrors and streams, takes the state saved before the last two frames
    and gets the first thread's bytes for them"""
    first = gpu_chain("stereo", "device")
    assert first.saved is not None and first.saved["t"] == SAVE_AT
    assert pkg.matcher_lib().orbx_thread_release_scratch() == pkg.ORBX_OK
    got = {}

    def worker():
        try:
            fr = S.stereo_frames()
            ch = K.Chain(K.GpuDeviceBackend(S.W, S.H, S.STEREO["nf"]), "stereo")
            ch.restore(first.saved, fr[SAVE_AT - 1])
            for l, r in fr[SAVE_AT:]:
                ch.step_stereo(l, r)
            got["digest"] = K.digest(ch)
            got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001  (shown by the assert below)
            got["error"] = repr(e)
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert "error" not in got, got["error"]
    assert got["rc"] == pkg.ORBX_OK and len(got["digest"]) > 0 and got["digest"] == K.digest(first, SAVE_AT)
