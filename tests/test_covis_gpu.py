"""GPU: covisibility through the Python entry points (update_connections, keyframe_culling, update_normal_and_depth, covisibility) on
every scene of tests/covis_scene.py.  Integer outputs equal the literal restatement tests/covis_ref.py, float outputs are bit-equal;
the combined call equals the three separate ones; two calls in a row on one thread with a regrow of the staging pair between them."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covis_ref as R        # noqa: E402
import covis_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu


def assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype and g.tobytes() == np.ascontiguousarray(w).tobytes()


def run_connections(pkg, sc):
    return pkg.update_connections(sc["table"], sc["queries"], th=sc["th"], cap=sc["cap"], counters=True)


def run_culling(pkg, sc):
    return pkg.keyframe_culling(sc["table"], sc["queries"], sc["monocular"], th_obs=sc["th_obs"])


@pytest.mark.parametrize("name", list(S.CONNECTION_CASES))
def test_update_connections_equals_the_restatement(pkg, name):
    sc = S.CONNECTION_CASES[name]()
    assert_same(run_connections(pkg, sc), S.expected_connections(sc))


@pytest.mark.parametrize("name", list(S.CULLING_CASES))
def test_keyframe_culling_equals_the_sequential_loop(pkg, name):
    sc = S.CULLING_CASES[name]()
    assert_same(run_culling(pkg, sc), S.expected_culling(sc))


@pytest.mark.parametrize("name", list(S.NORMAL_CASES))
def test_update_normal_and_depth_is_bit_equal(pkg, name):
    sc = S.NORMAL_CASES[name]()
    got = pkg.update_normal_and_depth(sc["table"])
    assert got.dtype == pkg.COVIS_NORMAL_DTYPE and got.tobytes() == R.update_normal_and_depth(sc["table"]).tobytes()


def test_outputs_are_optional(pkg):
    sc = S.CONNECTION_CASES["ties"]()
    ids, ws, n, cnt = pkg.update_connections(sc["table"], sc["queries"], th=sc["th"], cap=2)
    want = S.expected_connections(dict(sc, cap=2))
    assert cnt is None
    assert_same((ids, ws, n), want[:3])
    ids, ws, n, _ = pkg.update_connections(sc["table"], sc["queries"], th=sc["th"], cap=0)
    assert ids.shape == (1, 0) and n.tobytes() == want[2].tobytes()
    sk = S.CULLING_CASES["point_dies"]()
    nm, nr, v, pb = pkg.keyframe_culling(sk["table"], sk["queries"], sk["monocular"], point_bad=False)
    assert pb is None
    assert_same((nm, nr, v), S.expected_culling(sk)[:3])


@pytest.mark.parametrize("name", ["random", "random_long_lists", "point_dies"])
def test_combined_call_equals_the_three_separate_ones(pkg, name):
    sc = S.CULLING_CASES[name]()
    conn = dict(queries=sc["queries"], th=2, cap=9, counters=True)
    out = pkg.covisibility(sc["table"], connections=conn, culling=dict(queries=sc["queries"], monocular=sc["monocular"], th_obs=sc["th_obs"]), normals=True)
    assert_same(out["connections"], pkg.update_connections(sc["table"], sc["queries"], th=2, cap=9, counters=True))
    assert_same(out["connections"], S.expected_connections(dict(table=sc["table"], queries=sc["queries"], th=2, cap=9)))
    assert_same(out["culling"], run_culling(pkg, sc))
    assert_same(out["culling"], S.expected_culling(sc))
    assert out["normals"].tobytes() == pkg.update_normal_and_depth(sc["table"]).tobytes() == R.update_normal_and_depth(sc["table"]).tobytes()


def test_two_calls_in_a_row_with_a_regrow_between(pkg):
    """a small call on the thread's fresh staging pair, one that needs a larger pair (the global counter block and the radix buffers of
    K = COVIS_LDS_KEYFRAMES + 1), then the small one again on the regrown pair"""
    assert pkg.matcher_lib().orbx_thread_release_scratch() == 0
    small, big = S.CONNECTION_CASES["ties"](), S.CONNECTION_CASES["K_lds_plus_1"]()
    need = 3 * (S.LDS_KEYFRAMES + 1) * (4 + 16)
    assert need > (1 << 18)              # more than a new pair's first capacity
    want_small, want_big = S.expected_connections(small), S.expected_connections(big)
    cull = S.CULLING_CASES["chain"]()
    assert_same(run_connections(pkg, small), want_small)
    assert_same(run_connections(pkg, big), want_big)
    assert_same(run_connections(pkg, small), want_small)
    assert_same(run_culling(pkg, cull), S.expected_culling(cull))
    assert_same(run_connections(pkg, big), want_big)
    assert pkg.matcher_lib().orbx_thread_release_scratch() == 0
    assert_same(run_culling(pkg, cull), S.expected_culling(cull))
