"""GPU: no result of the loop map correction depends on what fresh scratch memory held.  The developer build's
orbx_debug_set_alloc_fill fills every new scratch block with a word before the library sees it; each case runs on a FRESH staging pair
(orbx_thread_release_scratch) with the fill off, with the word 1 and with the word 3, and the three results are identical and equal to
the restatement.  What could go wrong here: the owner array, which lives in device memory only and takes a minimum (k_mc_sim3 must
have set every entry first), and the keyframes of the spread that no level writes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapcorrect_ref as MR        # noqa: E402
import mapcorrect_scene as S       # noqa: E402
from test_mapcorrect_gpu import run_loop, run_spread      # noqa: E402

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


@pytest.mark.parametrize("name", ["q1", "scaled"])
def test_correct_loop(pkg, hooks, name):
    sc = S.loop_scene(name)
    got = three(pkg, lambda: [run_loop(pkg, sc)[k] for k in MR.LOOP_ARRAYS])
    assert got == [np.ascontiguousarray(S.loop_expected(name)[k]).tobytes() for k in MR.LOOP_ARRAYS]


def test_spread(pkg, hooks):
    sc = S.spread_scene("tree")
    got = three(pkg, lambda: [run_spread(pkg, sc)[k] for k in MR.SPREAD_ARRAYS])
    assert got == [np.ascontiguousarray(S.spread_expected("tree")[k]).tobytes() for k in MR.SPREAD_ARRAYS]
