"""The two sequences tests/track_chain.py is run over, the CPU chains on them (run once per process and left unchanged), the
conditions under which a device chain may be compared with them, and the distance of a chain's poses from the planted ones.

STEREO: synth.stereo_sequence(752, 480, 6, k = 11, step = 0.04), 1000 features, tracking_chain.poses behind world(): the first pose
is a rotation of 40 degrees and an offset, so that no pose of the sequence is a pure translation.  Six frames are the fewest that
hold what the chain can get wrong: frame 1 without a velocity, frames 2-3 with one, the key frame at t = 4 whose new points are
placed with an ESTIMATED pose, and frame 5 that tracks those points.  Both optimisations flag outliers and the local search
adds matches in every frame.

MONOCULAR: the first five left images of synth.stereo_sequence(752, 480, 6, k = 3, step = 0.8) (the rendered length sets the scene's
width, so it is part of the seed): one uniform sequence whose step is 20 of the stereo scene's (at 0.04 the Initializer refuses
frames 0 / 4 for their parallax and finds fewer than 100 matches for 0 / 12).  4000 features for the two initialisation frames
(2 x nFeatures), 2000 afterwards.  Initialised on frames 0 and 1, tracked on frames 2, 3 and 4: THREE tracked frames.
    Frame 2 is tracked exactly as the reference's tracking thread would: the initial points carry the distance ranges of before the
    scaling, isInFrustum refuses all of them, the local search adds nothing and the second optimisation sees the first one's inliers.
    Before frame 3 the scene calls Chain.recompute_ranges() - UpdateNormalAndDepth at the scaled positions, which in the reference is
    the mapper's work once a key frame adds an observation: A STATED STEP OF THE SCENE, not of the tracking thread - so that frames 3
    and 4 run the monocular local search and the second optimisation on real candidates (102 points in view, 18 and 17 matches added,
    2 outliers each).  Without it the tracked set only shrinks (59 -> 38 -> 29 inliers) and frame 4 is lost.
    Without the recompute, of the 120 (seed, step) pairs run - seeds 0-39 at steps 0.7 and 0.8, 0-27 at 0.75, 0-11 at 0.6 - thirteen sustain
    four frames, and each of those leaves CheckRT within 1e-5 of a threshold (about one pair in eight clears that margin).  At step 0.8
    the seeds 0 and 3 meet every condition; 3 is used: its CheckRT margin is the larger (1.8e-5 against 1.6e-5).  survey_mono() reruns
    that survey (about 2 s per pair)."""
import importlib
import time

import numpy as np

import init_scene
import track_chain as K
import tracking_chain as TC

W, H = 752, 480
STEREO = dict(T=6, k=11, step=0.04, nf=1000)
MONO = dict(T=5, recompute_at=3, rendered=6, k=3, step=0.8, nf_init=4000, nf_track=2000)
EDGE = 3                # a count must clear its threshold by more than this: one borderline match moves a count by one
_cache = {}


def _synth():
    return importlib.import_module(K.PKG + ".synth")


def stereo_frames():
    if "stereo" not in _cache:
        _cache["stereo"] = _synth().stereo_sequence(W, H, STEREO["T"], k=STEREO["k"], step=STEREO["step"])[0]
    return _cache["stereo"]


def mono_images():
    if "mono" not in _cache:
        _cache["mono"] = [f[0] for f in _synth().stereo_sequence(W, H, MONO["rendered"], k=MONO["k"], step=MONO["step"])[0]][:MONO["T"]]
    return _cache["mono"]


def world():
    """the stereo chain's world frame seen from the first camera: a rotation of 40 degrees and an offset.  With the first pose at the
    identity every pose of the sequence is a pure translation, and products of pure translations commute: a transposed velocity, or
    a camera centre taken for a translation, would go unnoticed."""
    a = np.array([0.3, 1.0, 0.2])
    a /= np.linalg.norm(a)
    th = np.deg2rad(40.0)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Wd = np.eye(4)
    Wd[:3, :3] = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    Wd[:3, 3] = (1.5, -0.7, 2.0)
    return Wd


def stereo_poses():
    """the planted Tcw of every frame: tracking_chain.poses (the camera advances along its own +X) behind world()"""
    return [(P.astype(np.float64) @ world()).astype(np.float32) for P in TC.poses(STEREO["T"], STEREO["step"])]


def run(mode, backend_cls, mutate=None, upto=None, **kw):
    """a chain of `mode` on a fresh backend (stereo: over the first `upto` frames)"""
    t0 = time.perf_counter()
    if mode == "stereo":
        ch = K.run_stereo(backend_cls(W, H, STEREO["nf"]), stereo_frames()[:upto], stereo_poses()[0], mutate=mutate, **kw)
    else:
        ch = K.run_mono(backend_cls(W, H, MONO["nf_track"]), mono_images(), MONO["k"], MONO["nf_init"], MONO["nf_track"], mutate=mutate, recompute_at=MONO["recompute_at"])
    ch.seconds = time.perf_counter() - t0
    return ch


def survey_mono(steps=(0.6, 0.7, 0.75, 0.8), seeds=range(40), rendered=6):
    """the seed survey of the docstring: per (step, seed) the initialisation's counts and margins and the inliers of every frame the CPU
    chain tracks before it is lost.  Not run by a test: python -c "import track_scene as S; [print(x) for x in S.survey_mono()]" """
    for step in steps:
        for k in seeds:
            imgs = [f[0] for f in _synth().stereo_sequence(W, H, rendered, k=k, step=step)[0]]
            ch = K.run_mono(K.CpuBackend(W, H, MONO["nf_track"]), imgs, k, MONO["nf_init"], MONO["nf_track"])
            r = [e["out"]["info"] for e in ch.trace if e["stage"] == "initialize"]
            yield dict(step=step, k=k, init={a: ch.init.get(a) for a in ("ok", "matches", "triangulated", "why")},
                       margin_chi=r[0]["margin_chi"] if r else None, margin_rt=r[0]["margin_rt"] if r else None,
                       inliers=[c["inliers"] for c in ch.frames], lost=ch.lost)


def cpu_chain(mode):
    if ("cpu", mode) not in _cache:
        _cache[("cpu", mode)] = run(mode, K.CpuBackend)
    return _cache[("cpu", mode)]


# ---------------------------------------------------------------------------------------------------- poses against the planted ones
def pose_errors(mode, ch):
    """stereo: the largest |t - t_true| entry in metres and the largest |R - R_true| entry over the frames.
    mono (the scale is fixed by the median depth only): the largest entry of t_k / |t_k| - (-1, 0, 0), the largest
    | |t_k| / |t_1| - k |, and the largest |R - I| entry, over the frames k >= 1"""
    if mode == "stereo":
        P = stereo_poses()
        rot = max(float(np.abs(T[:3, :3].astype(np.float64) - P[t][:3, :3]).max()) for t, T in enumerate(ch.poses))
        return dict(translation=max(float(np.abs(T[:3, 3].astype(np.float64) - P[t][:3, 3]).max()) for t, T in enumerate(ch.poses)), rotation=rot)
    rot = max(float(np.abs(T[:3, :3].astype(np.float64) - np.eye(3)).max()) for T in ch.poses)
    t = [T[:3, 3].astype(np.float64) for T in ch.poses]
    n1 = np.linalg.norm(t[1])
    return dict(direction=max(float(np.abs(x / np.linalg.norm(x) - np.array([-1.0, 0, 0])).max()) for x in t[1:]),
                ratio=max(abs(float(np.linalg.norm(x) / n1) - k) for k, x in enumerate(t) if k >= 1), rotation=rot)


# The largest errors of the CPU chains, measured on the CPU (tests/test_track_chain_cpu.py asserts that they are what the CPU chains
# show, to the two digits given); a device chain must stay within 4 x these: the factor allows for a chain that diverged by one
# borderline match.  Never taken from a GPU run.
CPU_ERRORS = {
    "stereo": dict(translation=5.7e-3, rotation=4.1e-4),              # metres (the true step is 0.0215 per frame); entries of R
    "mono": dict(direction=9.4e-3, ratio=3.4e-2, rotation=6.9e-4),
}


def within_bounds(mode, ch):
    e = pose_errors(mode, ch)
    return all(e[k] <= 4 * CPU_ERRORS[mode][k] for k in e), e


# ---------------------------------------------------------------------------------------------------- the conditions
def optimize_margins(ch):
    """per PoseOptimization call of a chain whose trace carries the restatement (the CPU chain): the smallest margin of its rounds"""
    return [(e["frame"], e["stage"], min(tr["min_margin"] for tr in e["out"]["info"]["trace"])) for e in ch.trace if e["stage"].startswith("optimize")]


def assert_counts(mode, ch):
    """the rules every chain must keep meeting, with no count at a decision's edge"""
    assert ch.lost is None, ch.lost
    if mode == "mono":
        r = ch.init
        assert r["ok"] and r["matches"] >= 100 + EDGE and r["triangulated"] >= 100 + EDGE and r["tracked"] >= 100 + EDGE and r["median_depth"] > 0, r
        assert len(ch.frames) == MONO["T"] - 2 >= 2
    else:
        assert len(ch.frames) == STEREO["T"] - 1
    for c in ch.frames:
        assert c["proj"] >= 20 + EDGE and c["matches_map"] >= 10 + EDGE and c["inliers"] >= 30 + EDGE, c


def assert_init_margins(r):
    """init_scene.assert_conditions on the restatement's answer for the chain's own matches"""
    M = init_scene.MARGIN
    assert r["margin_chi"] > M and r["margin_rt"] > M, (r["margin_chi"], r["margin_rt"])
    assert not abs(float(r["RH"]) - 0.40) <= 1e-4 and abs(float(r["parallax"]) / 1.0 - 1.0) > 1e-3, (r["RH"], r["parallax"])
    assert not any(bool(e) for e in r.get("equalities", []))
