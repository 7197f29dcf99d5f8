"""CPU: the tracking chains of tests/track_chain.py on the restatements alone (the C oracle's extractor and matchers, init_ref,
pose_ref) over the scenes of tests/track_scene.py - the conditions under which tests/test_track_chain_gpu.py may demand equality,
the mutations, and the poses against the planted ones.  No GPU.

MEASURED HERE, on the CPU chains (the bounds a device chain is held to are 4 x these, track_scene.CPU_ERRORS):
    stereo (k = 11, T = 6, step 0.04, 1000 features, the first pose rotated by 40 degrees; 2 s with the oracle's extraction)
        per frame 167-199 projection matches, 2-12 outliers at the first optimisation, 10-28 matches added by the local search,
        1-4 outliers at the second, 154-196 inliers; the smallest distance of an edge from its threshold 2.0e-2
        largest translation error 5.7e-3 m (true step 0.0215 m per frame), largest rotation-entry error 4.1e-4
    mono (k = 3 of a 6-frame rendering, step 0.8, 4000 / 2000 features; 2 s): THREE tracked frames sustained, the ranges recomputed
        before the second (track_scene)
        initialisation: 149 matches, F chosen (RH 0.19), 148 good of 148 inliers, parallax 2.14 deg, 148 triangulated, CheckRT's margin
        1.8e-5, median depth 24.8; tracked: 69, 42 and 37 projection matches, 10, 4 and 3 outliers at the first optimisation, 0, 18 and
        17 matches added by the local search, 0, 2 and 2 outliers at the second, 59, 54 and 49 inliers
        translation direction within 9.4e-3 of (-1, 0, 0), |t_k| / |t_1| within 3.4e-2 of k, rotation entries within 6.9e-4
        In frame 2 the local search adds NOTHING and the second optimisation flags nothing: the reference scales the points by 1 / 24.8
        and leaves their distance ranges (see track_chain), so isInFrustum refuses every point by its range.  That is asserted below as
        what the transcription gives; frames 3 and 4 follow the scene's stated recompute of the ranges and meet "the local search adds
        matches" and "an outlier at each optimisation" on the monocular path too."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_chain as K         # noqa: E402
import track_scene as S         # noqa: E402
from test_poseopt_gpu import MARGIN     # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _oracle(oracle):
    return oracle


def test_stereo_chain_meets_the_conditions():
    ch = S.cpu_chain("stereo")
    S.assert_counts("stereo", ch)
    assert all(m > MARGIN for _, _, m in S.optimize_margins(ch)), S.optimize_margins(ch)
    assert all(c["outliers_motion"] >= 1 and c["outliers_local"] >= 1 and c["local"] >= 1 + S.EDGE for c in ch.frames), ch.frames
    # the key frame at t = 4 placed points with the estimated pose, and frame 5 tracked them
    sizes = [e["out"]["map_size"] for e in ch.trace if e["stage"] == "end"]
    assert sizes[4] > sizes[3] and ch.frames[-1]["matches_map"] > ch.frames[-2]["matches_map"]
    print("stereo: %.1f s; %s" % (ch.seconds, ch.frames))


def test_mono_chain_meets_the_conditions():
    ch = S.cpu_chain("mono")
    S.assert_counts("mono", ch)
    r = [e for e in ch.trace if e["stage"] == "initialize"][0]["out"]["info"]
    S.assert_init_margins(r)
    assert r["model"] == 1 and r["best_good"] >= 50 + S.EDGE
    assert all(m > MARGIN for _, _, m in S.optimize_margins(ch)), S.optimize_margins(ch)
    first, rest = ch.frames[0], ch.frames[1:]
    assert first["in_view"] == 0 and first["local"] == 0 and first["outliers_local"] == 0             # the stale ranges: see the docstring
    assert len(rest) == 2 and all(c["in_view"] > 50 and c["local"] >= 1 + S.EDGE and c["outliers_local"] >= 1 for c in rest), rest
    assert all(c["outliers_motion"] >= 1 for c in ch.frames)
    assert [e["frame"] for e in ch.trace if e["stage"] == "recompute_ranges"] == [S.MONO["recompute_at"]]
    print("mono: %.1f s; %s; %s" % (ch.seconds, ch.init, ch.frames))


@pytest.mark.parametrize("mode", ["stereo", "mono"])
def test_poses_follow_the_planted_ones(mode):
    e = S.pose_errors(mode, S.cpu_chain(mode))
    print(mode, e)
    for k, v in e.items():                     # the recorded figures are the measured ones, rounded up to two digits
        assert 0.9 * S.CPU_ERRORS[mode][k] <= v <= S.CPU_ERRORS[mode][k], (k, v)


# mutation -> (scene, the first entry A BACKEND PRODUCED (track_chain.DEVICE_STAGES) that differs from the unmutated chain; None: no
# scene notices it).  What the bookkeeping logs of itself (the velocity, the point table after a sweep) differs under every mutation and
# proves nothing, so it is not compared.
#   velocity_transposed moves the prediction of frames 2-5 by 0.9 - 1.6 cm (the true step is 2.15 cm; with the first pose at the identity
#       the two products would be equal).  The 7-pixel window absorbs that: SearchByProjection returns the SAME matches in every frame, and
#       the join shows only in the pose the solver reaches from the other start (entries differ by up to 3.5e-5, no flag differs).  So the
#       scene notices this mistake in the solver's bits, not in a count; a scene that loses matches to it would need a faster camera.
#   mono_outliers_nulled_in_local_map is NOT noticed, and no monocular scene of this chain can notice it: without a key frame or a
#       mapper nothing reads the point table between TrackLocalMap and the sweep at the end of Track(), so both orders leave the same
#       frame, also in frames 3 and 4 whose second optimisation does flag outliers.  The line is transcribed where the reference has it.
NOTICED = {
    "sigma2_of_level_0": ("stereo", (1, "optimize_motion")),
    "keep_outliers_before_local_search": ("stereo", (1, "local")),
    "velocity_transposed": ("stereo", (2, "optimize_motion")),
    "stereo_edges_without_ur": ("stereo", (1, "optimize_motion")),
    "mono_outliers_nulled_in_local_map": ("mono", None),
}


@pytest.mark.parametrize("name", list(K.MUTATIONS))
def test_the_scenes_notice_the_mutations(name):
    mode, where = NOTICED[name]
    base, mutated = S.cpu_chain(mode), S.run(mode, K.CpuBackend, mutate=name)
    d = K.first_difference(base, mutated, common=True, stages=K.DEVICE_STAGES)
    print(name, "first differs at", d, "lost", mutated.lost)
    assert d == where, (name, d)
    if name == "velocity_transposed":
        pred = [np.abs(x["out"]["Tcw"] - y["out"]["Tcw"]).max() for x, y in zip(base.trace, mutated.trace) if x["stage"] == "predict" and x["frame"] >= 2]
        same = [(x["out"]["match"] == y["out"]["match"]).all() for x, y in zip(base.trace, mutated.trace) if x["stage"] == "project"]
        assert len(pred) == 4 and min(pred) > 5e-3 and all(same), (pred, same)          # what the comment above says


def test_mutations_are_complete():
    assert set(NOTICED) == set(K.MUTATIONS) and len(K.MUTATIONS) >= 5
