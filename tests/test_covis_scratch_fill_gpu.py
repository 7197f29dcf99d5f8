"""GPU: no covisibility result depends on what fresh scratch memory held.  The developer build's
orbx_debug_set_alloc_fill fills every new scratch block with a word before the library sees it; each case runs on a FRESH staging pair
(orbx_thread_release_scratch) with the fill off, with the word 1 and with the word 3, and the three results are identical and equal to
the restatement.  The cases: K = COVIS_LDS_KEYFRAMES + 1, where the counters are added into a global block that the call itself must
zero and the sort runs between global buffers; and a culling case, whose set of culled keyframes starts in LDS."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covis_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
WORDS = (1, 3)


def three(pkg, run):
    L = pkg.matcher_lib()
    assert L._orbx_developer
    outs, stats = [], []
    for word in (None,) + WORDS:
        assert L.orbx_thread_release_scratch() == 0
        pkg.debug_set_alloc_fill(word is not None, word or 0)
        try:
            outs.append([np.ascontiguousarray(a).tobytes() for a in run()])
            stats.append(pkg.debug_alloc_fill_stats())
        finally:
            pkg.debug_set_alloc_fill(0)
    assert L.orbx_thread_release_scratch() == 0
    assert stats[0] == (0, 0), stats
    for word, out, st in zip(WORDS, outs[1:], stats[1:]):
        assert out == outs[0], "differs with fresh scratch filled with %d" % word
        assert st[0] >= 2 and st[1] >= 8, (word, st)      # the staging pair's two blocks were filled
    return outs[0]


def test_global_counter_path(pkg, hooks):
    sc = S.CONNECTION_CASES["K_lds_plus_1"]()
    got = three(pkg, lambda: pkg.update_connections(sc["table"], sc["queries"], th=sc["th"], cap=sc["cap"], counters=True))
    assert got == [np.ascontiguousarray(a).tobytes() for a in S.expected_connections(sc)]


def test_long_order_path(pkg, hooks):
    sc = S.CONNECTION_CASES["long_order"]()
    got = three(pkg, lambda: pkg.update_connections(sc["table"], sc["queries"], th=sc["th"], cap=sc["cap"], counters=True))
    assert got == [np.ascontiguousarray(a).tobytes() for a in S.expected_connections(sc)]


@pytest.mark.parametrize("name", ["point_dies", "random"])
def test_culling(pkg, hooks, name):
    sc = S.CULLING_CASES[name]()
    got = three(pkg, lambda: pkg.keyframe_culling(sc["table"], sc["queries"], sc["monocular"], th_obs=sc["th_obs"]))
    assert got == [np.ascontiguousarray(a).tobytes() for a in S.expected_culling(sc)]
