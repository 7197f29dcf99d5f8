"""GPU: k_new_points and the chain orbl_create_new_map_points against the numpy restatement tests/newpoints_ref.py on every scene of
tests/newpoints_scene.py.  status, x y z and cos_rays are compared byte for byte; cos_stereo, the one value that goes through the
device's atan2f / cosf, within STEPS float steps of the double evaluation rounded to float (the scenes' conditions, asserted in
tests/test_newpoints_cpu.py, say that no decision changes within that allowance).  Also: two runs give the same bytes, the batch
equals the single calls, the chain equals the restatement's chain AND a loop of orbm_search_for_triangulation + orbl_triangulate with
the flags updated on the host, a second host thread and fresh scratch filled with two different words change nothing."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import newpoints_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
STEPS = 4
EXACT = ("x", "y", "z", "status", "cos_rays", "reserved")


def kf_of(pkg, k):
    return pkg.newpoints_keyframe(k["view"], k["kp"], k["st"], k["sf"], k["sig2"])


def run(pkg, sc):
    return pkg.triangulate_new_points(kf_of(pkg, sc["kf1"]), kf_of(pkg, sc["kf2"]), sc["pairs"])


def cos_steps(got, ref):
    if got.size == 0:
        return 0
    return int(np.abs(got["cos_stereo"].view(np.int32).astype(np.int64) - ref["cos_stereo"].view(np.int32).astype(np.int64)).max())


def assert_rows(got, ref, what):
    assert got.shape == ref.shape
    for f in EXACT:
        assert got[f].tobytes() == ref[f].tobytes(), (what, f, np.flatnonzero((got[f] != ref[f]).reshape(len(got.reshape(-1)), -1).any(1))[:8])
    s = cos_steps(got, ref)
    print("%s: cos_stereo at most %d float steps from the restatement (allowed: %d)" % (what, s, STEPS))
    assert s <= STEPS, (what, s)
    return s


@pytest.mark.parametrize("name", list(S.CASES))
def test_device_equals_the_restatement(pkg, name):
    sc = S.case(name)
    ref, _ = S.reference(name)
    got, nnew = run(pkg, sc)
    assert_rows(got, ref, name)
    assert nnew == (ref["status"] >= 0).sum()


def test_two_runs_give_the_same_bytes(pkg):
    for name in ("n257", "stereo_stereo", "raw_differs"):
        a, b = run(pkg, S.case(name)), run(pkg, S.case(name))
        assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]


def test_batch_equals_the_single_calls(pkg):
    """four pairs of keyframes in one launch, an empty pair second, offsets that are no multiple of 64"""
    scs = [S.case(n) for n in S.BATCH]
    off = np.cumsum([0] + [len(sc["pairs"]) for sc in scs]).astype(np.int32)
    assert off[1] == off[2] and all(o % 64 for o in off[1:])
    pts, nnew = pkg.triangulate_new_points_batch([kf_of(pkg, sc["kf1"]) for sc in scs], [kf_of(pkg, sc["kf2"]) for sc in scs], off,
                                                 np.concatenate([sc["pairs"] for sc in scs]))
    for p, sc in enumerate(scs):
        one, n1 = run(pkg, sc)
        assert pts[off[p]:off[p + 1]].tobytes() == one.tobytes() and nnew[p] == n1, S.BATCH[p]
    # the current keyframe given once for every pair (its arrays go up once): two neighbours of a chain scene
    ch = S.chain("chain_stereo")
    cur = kf_of(pkg, ch["cur"])
    r = S.chain_reference("chain_stereo")
    prs = [np.stack([np.flatnonzero(r["match_q"][i] >= 0), r["match_q"][i][r["match_q"][i] >= 0]], axis=1) for i in range(2)]
    off = np.array([0, len(prs[0]), len(prs[0]) + len(prs[1])], np.int32)
    pts, nnew = pkg.triangulate_new_points_batch([cur, cur], [kf_of(pkg, ch["nbs"][i]["kf"]) for i in range(2)], off, np.concatenate(prs))
    for i in range(2):
        one, n1 = pkg.triangulate_new_points(cur, kf_of(pkg, ch["nbs"][i]["kf"]), prs[i])
        assert pts[off[i]:off[i + 1]].tobytes() == one.tobytes() and nnew[i] == n1


def neighbours_of(pkg, sc):
    return [pkg.newpoints_neighbour(kf_of(pkg, nb["kf"]), nb["cd"], nb["cf"], nb["nqs"], nb["qi"], nb["ncs"], nb["ci"], nb["F12"], nb["ex"], nb["ey"],
                                    nb["median"]) for nb in sc["nbs"]]


def run_chain(pkg, sc):
    return pkg.create_new_map_points(kf_of(pkg, sc["cur"]), sc["qd"], sc["qf"], neighbours_of(pkg, sc), sc["monocular"])


def chain_bytes(r):
    return b"".join(np.ascontiguousarray(r[k]).tobytes() for k in ("match_q", "points", "nmatches", "nnew", "skipped", "q_flags"))


@pytest.mark.parametrize("name", list(S.CHAINS))
def test_chain_equals_the_restatements_chain(pkg, name):
    sc, ref = S.chain(name), S.chain_reference(name)
    got = run_chain(pkg, sc)
    for k in ("match_q", "nmatches", "nnew", "skipped", "q_flags"):
        assert (got[k] == ref[k]).all(), (name, k)
    assert_rows(got["points"], ref["points"], name)


@pytest.mark.parametrize("name", list(S.CHAINS))
def test_chain_equals_a_host_loop_over_the_two_entry_points(pkg, name):
    """orbm_search_for_triangulation + orbl_triangulate per neighbour, the flags updated on the host in between: the chain must give
    the same bytes.  A query that neighbour 0 accepted and neighbour 1 would match again (scene condition (a)) makes this fail when
    the device does not clear the flag."""
    sc = S.chain(name)
    cur, flags = kf_of(pkg, sc["cur"]), sc["qf"].copy()
    nq, nn = len(sc["qf"]), len(sc["nbs"])
    want = {"match_q": np.full((nn, nq), -1, np.int32), "points": np.zeros((nn, nq), pkg.NEWPOINT_DTYPE), "nmatches": np.zeros(nn, np.int32),
            "nnew": np.zeros(nn, np.int32), "skipped": np.zeros(nn, bool)}
    for i, nb in enumerate(sc["nbs"]):
        if not pkg.baseline_ok(sc["cur"]["view"], nb["kf"]["view"], sc["monocular"], nb["median"]):
            want["skipped"][i] = True
            want["points"]["status"][i] = -9
            continue
        n, mq = pkg.search_for_triangulation(sc["cur"]["kp"], sc["qd"], flags, nb["kf"]["kp"], nb["cd"], nb["cf"], nb["nqs"], nb["qi"], nb["ncs"], nb["ci"],
                                             nb["F12"], nb["ex"], nb["ey"], nb["kf"]["sf"], nb["kf"]["sig2"], 50, False)
        idx1 = np.flatnonzero(mq >= 0)
        rows, nnew = pkg.triangulate_new_points(cur, kf_of(pkg, nb["kf"]), np.stack([idx1, mq[idx1]], axis=1))
        want["match_q"][i], want["nmatches"][i], want["nnew"][i] = mq, n, nnew
        want["points"]["status"][i] = -10
        want["points"][i, idx1] = rows
        flags[idx1[rows["status"] >= 0]] &= 0xFE
    want["q_flags"] = flags
    got = run_chain(pkg, sc)
    for k in ("match_q", "points", "nmatches", "nnew", "skipped", "q_flags"):
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (name, k)
    assert (flags != sc["qf"]).sum() == want["nnew"].sum() > 0


def test_second_host_thread_and_scratch_release(pkg):
    sc, ch = S.case("n257"), S.chain("chain_stereo")
    base = run(pkg, sc)[0].tobytes() + chain_bytes(run_chain(pkg, ch))
    out = {}

    def worker():
        try:
            out["a"] = run(pkg, sc)[0].tobytes() + chain_bytes(run_chain(pkg, ch))
            out["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
            out["b"] = run(pkg, sc)[0].tobytes() + chain_bytes(run_chain(pkg, ch))
            pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001
            out["err"] = repr(e)
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert "err" not in out, out
    assert out["rc"] == 0 and out["a"] == base and out["b"] == base


def test_results_do_not_depend_on_what_fresh_scratch_held(pkg, hooks):
    """the developer build fills every new scratch block with a word: 1, then 3; the rows are those of zeroed scratch"""
    L = pkg.matcher_lib()
    assert L._orbx_developer
    sc, ch = S.case("n65"), S.chain("chain_mono")
    outs = []
    try:
        for word in (None, 1, 3):
            assert L.orbx_thread_release_scratch() == 0
            pkg.debug_set_alloc_fill(word is not None, word or 0)
            outs.append(run(pkg, sc)[0].tobytes() + chain_bytes(run_chain(pkg, ch)))
            if word is not None:
                st = pkg.debug_alloc_fill_stats()
                assert st[0] >= 2, st
    finally:
        pkg.debug_set_alloc_fill(0)
        L.orbx_thread_release_scratch()
    assert outs[1] == outs[0] and outs[2] == outs[0]
    assert_rows(np.frombuffer(outs[0][:65 * 32], pkg.NEWPOINT_DTYPE), S.reference("n65")[0], "n65 on filled scratch")


def test_error_returns_leave_clean_outputs(pkg):
    ch = S.chain("chain_stereo")
    cur, nbs = kf_of(pkg, ch["cur"]), neighbours_of(pkg, ch)
    bad = dict(ch["nbs"][1])
    bad["ci"] = bad["ci"].copy()
    bad["ci"][1] = bad["ci"][0]            # a candidate listed twice
    nb_bad = pkg.newpoints_neighbour(kf_of(pkg, bad["kf"]), bad["cd"], bad["cf"], bad["nqs"], bad["qi"], bad["ncs"], bad["ci"], bad["F12"], bad["ex"],
                                     bad["ey"], bad["median"])
    for lst, status in (([nbs[0], nb_bad], pkg.ORBX_ERR_ARG), ([nbs[0]] * 33, pkg.ORBX_ERR_UNSUPPORTED)):
        with pytest.raises(pkg.OrbxError) as e:
            pkg.create_new_map_points(cur, ch["qd"], ch["qf"], lst, False)
        assert e.value.status == status
    got = run_chain(pkg, ch)               # and the thread's scratch still works
    assert (got["match_q"] == S.chain_reference("chain_stereo")["match_q"]).all()
