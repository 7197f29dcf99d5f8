"""GPU: no local map result depends on what fresh device memory held.  The developer build's
orbx_debug_set_alloc_fill fills every new scratch block with a word before the library sees it; each case runs on a FRESH handle - its
snapshot, state and frame blocks are all new - with the fill off, with the word 1 and with the word 3, and the three results are
identical and equal to the restatement.  The cases: K = COVIS_LDS_KEYFRAMES + 1, where the counters are added into a global row that
the call itself must zero; the random scene, two frames in a row (the state block starts filled, not idle); and an empty frame, whose
lists have length 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_ref as LR        # noqa: E402
import localmap_scene as S       # noqa: E402
from test_localmap_gpu import got_bytes, run_frame, set_scene      # noqa: E402

pytestmark = pytest.mark.gpu
WORDS = (1, 3)


def three(pkg, run):
    assert pkg.matcher_lib()._orbx_developer
    outs, stats = [], []
    for word in (None,) + WORDS:
        pkg.debug_set_alloc_fill(word is not None, word or 0)
        try:
            outs.append(run())
            stats.append(pkg.debug_alloc_fill_stats())
        finally:
            pkg.debug_set_alloc_fill(0)
    assert stats[0] == (0, 0), stats
    for word, out, st in zip(WORDS, outs[1:], stats[1:]):
        assert out == outs[0], "differs with fresh memory filled with %d" % word
        assert st[0] >= 5, (word, st)      # snapshot + mirror, state, frame block + mirror
    return outs[0]


def frames(pkg, sc, n):
    with pkg.LocalMap() as lm:
        set_scene(lm, sc)
        return [got_bytes(run_frame(lm, sc)) for _ in range(n)]


@pytest.mark.parametrize("name", ["K_lds_plus_1", "random", "m_0"])
def test_fresh_memory_does_not_show(pkg, hooks, name):
    want = LR.result_bytes(S.expected(name))
    assert three(pkg, lambda: frames(pkg, S.scene(name), 2)) == [want, want]
