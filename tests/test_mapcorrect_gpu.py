"""GPU: the loop map correction (orbr_correct_loop, orbr_spread_global_ba through the package) against the literal restatement
tests/mapcorrect_ref.py on every scene of tests/mapcorrect_scene.py: every output array byte for byte.  The tolerance is zero: no sum
here has a free order, there is no transcendental, and the double sqrt and divisions of the kernels round as the host's do.  Two runs
give the same bytes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapcorrect_ref as MR        # noqa: E402
import mapcorrect_scene as S       # noqa: E402

pytestmark = pytest.mark.gpu


def run_loop(pkg, sc):
    return pkg.correct_loop_map(sc["table"], sc["queries"], sc["cur"], sc["Tiw"], sc["Scw"])


def run_spread(pkg, sc):
    off, child = S.child_lists(sc)
    return pkg.spread_global_ba(sc["Tcw"], sc["TcwGBA"], sc["kf_in_gba"], off, child, sc["origins"], sc["pos"], sc["posGBA"], sc["pt_in_gba"], sc["ref_kf"],
                                sc["bad"])


def differing(got, want, k):
    g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
    if g.tobytes() == w.tobytes():
        return None
    rows = [i for i in range(len(w)) if g[i].tobytes() != w[i].tobytes()]
    return "%s: %d of %d rows differ, first %d: %r != %r" % (k, len(rows), len(w), rows[0], g[rows[0]], w[rows[0]])


@pytest.mark.parametrize("name", S.LOOP_SCENES)
def test_correct_loop_equals_the_restatement(pkg, name):
    got, want = run_loop(pkg, S.loop_scene(name)), S.loop_expected(name)
    assert got["normals"].dtype == MR.NORMAL_DTYPE and got["corrected"].dtype == MR.SIM3_DTYPE
    bad = [d for d in (differing(got, want, k) for k in MR.LOOP_ARRAYS) if d]
    assert not bad, "\n".join(bad)
    again = run_loop(pkg, S.loop_scene(name))
    assert all(again[k].tobytes() == got[k].tobytes() for k in MR.LOOP_ARRAYS)


@pytest.mark.parametrize("name", S.SPREAD_SCENES)
def test_spread_equals_the_restatement(pkg, name):
    got, want = run_spread(pkg, S.spread_scene(name)), S.spread_expected(name)
    bad = [d for d in (differing(got, want, k) for k in MR.SPREAD_ARRAYS) if d]
    assert not bad, "\n".join(bad)
    assert got["levels"] == want["levels"]
    again = run_spread(pkg, S.spread_scene(name))
    assert all(again[k].tobytes() == got[k].tobytes() for k in MR.SPREAD_ARRAYS) and again["levels"] == got["levels"]


def test_empty_map(pkg):
    """no keyframe and no point: nothing to do, no device touched; points alone (every reference keyframe -1): all undefined or mPosGBA"""
    z = np.zeros
    out = pkg.spread_global_ba(z((0, 4, 4), np.float32), z((0, 4, 4), np.float32), z(0, np.uint8), z(1, np.int32), z(0, np.int32), z(0, np.int32),
                               z((0, 3), np.float32), z((0, 3), np.float32), z(0, np.uint8), z(0, np.int32), z(0, np.uint8))
    assert out["levels"] == 0 and len(out["status"]) == 0
    pos, gba = np.arange(9, dtype=np.float32).reshape(3, 3), np.arange(9, dtype=np.float32).reshape(3, 3) + 100
    out = pkg.spread_global_ba(z((0, 4, 4), np.float32), z((0, 4, 4), np.float32), z(0, np.uint8), z(1, np.int32), z(0, np.int32), z(0, np.int32),
                               pos, gba, np.array([0, 1, 1], np.uint8), np.full(3, -1, np.int32), np.array([0, 0, 1], np.uint8))
    assert list(out["status"]) == [MR.SPREAD_UNDEFINED, MR.SPREAD_GBA, MR.SPREAD_UNTOUCHED]
    assert out["pos"].tobytes() == np.stack([pos[0], gba[1], pos[2]]).tobytes()
