"""GPU: k_pnp_ransac / k_pnp_refine / k_pnp_select (orbp_*, csrc/orbx_pnp.hip) against the restatement tests/pnp_ref.py on every
scene of tests/pnp_scene.py.

No operation on the path is implementation-defined: with -ffp-contract=off it is correctly rounded double and float + - * / sqrt,
fabs and comparisons, integer counts (ballot + popcount), and no floating-point value is combined across lanes.  So the demand is
BYTE EQUALITY of every output the C ABI returns - counts, the double models, the float poses, the chosen approximations, all
flags, the refined counts, the info record, the returned and the kept flags - a NaN equal to a NaN.  The conditions under which
the scenes were chosen (few borderline evaluations, no deciding count within its borderline count of its comparand) are asserted
in tests/test_pnp_cpu.py on the restatement alone; they are not needed for equality, they say that a one-ulp difference of the
device would show as a different float, not be hidden behind an unchanged count."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pnp_ref as R         # noqa: E402
import pnp_scene as S       # noqa: E402

pytestmark = pytest.mark.gpu
_runs = {}
KEYS = ("counts", "models", "tcws", "choices", "flags", "refined_counts", "inliers", "best_flags") + R.INFO_DTYPE.names


def call(pkg, sc):
    n = len(sc["corrs"])
    return pkg.pnp_ransac_batch(sc["corrs"], [0, n], S.problem(sc), sc["sets"], [0, len(sc["sets"])], sc["prior_best_flags"])[0]


def run(pkg, name):
    """one single call per scene, shared by the tests"""
    if name not in _runs:
        _runs[name] = call(pkg, S.case(name))
    return _runs[name]


def same_bytes(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in KEYS)


def as_lockstep(o):
    """the dict of pnp_ransac_batch in the shape pnp_scene.assert_equals_restatement takes"""
    return dict(o, info=o, rcounts=o["refined_counts"])


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernels_equal_the_restatement(pkg, name):
    o, r = run(pkg, name), S.reference(name)
    S.assert_equals_restatement(as_lockstep(o), r, full=False)
    print("%s: hit %d after %d iterations, best %d with %d, refined %d, pose %d" % (name, o["hit_iteration"], o["iterations_run"],
                                                                                   o["best_iteration"], o["best_inliers"], o["refined_inliers"], o["pose"]))


def test_two_runs_give_the_same_bytes(pkg):
    for name in ("hit_60", "n_1100", "duplicate", "two_calls"):
        assert same_bytes(call(pkg, S.case(name)), run(pkg, name)), name


def test_batch_equals_the_single_calls(pkg):
    b = S.batch(S.BATCH_3)
    outs = pkg.pnp_ransac_batch(b["corrs"], b["offsets"], b["problems"], b["sets"], b["set_offsets"], b["prior"])
    assert len(outs) == 4
    e = outs[1]                                                    # the empty problem
    assert (e["n"], e["iterations"], e["hit_iteration"], e["best_iteration"], e["no_more"], e["pose"]) == (0, 0, -1, -1, 1, 0) and not e["Tcw"].any()
    for o, name in zip([outs[0]] + outs[2:], S.BATCH_3):
        assert same_bytes(o, run(pkg, name)), name
    assert outs[2]["iterations"] == 0 and outs[2]["n"] == 9 and outs[2]["no_more"] == 1          # n_9: correspondences but no iteration


def sentinel(count, dtype):
    """an output array whose every byte is 0xA5: what a call did not write still reads so"""
    return np.full(count * np.dtype(dtype).itemsize, 0xA5, np.uint8).view(dtype)


def untouched(a):
    return bool((np.ascontiguousarray(a).view(np.uint8) == 0xA5).all())


def test_batch_whose_first_offset_is_not_zero(pkg):
    """the C ABI called on problems 1 .. of the four-problem batch: offsets + 1, set_offsets + 1, problems + 1, B - 1, the arrays'
    base pointers as in the full call.  Then offsets[0] = 60 and set_offsets[0] = 35 (p0, h0 of csrc/orbx_pnp.hip).  Every output
    indexed by a correspondence or a set lands where the full call puts it and equals the single call's; refined_counts, flags
    and infos are counted from this call's first problem; no byte of problem 0's ranges and none behind the used ranges is written"""
    b = S.batch(S.BATCH_3)
    off, soff, B = b["offsets"], b["set_offsets"], len(b["problems"])
    p0, h0, np_, nh = int(off[1]), int(soff[1]), int(off[B]), int(soff[B])
    assert B == 4 and p0 == 60 and h0 == 35 and nh > h0
    sets = np.ascontiguousarray(b["sets"], np.int32)
    nfl = [int(soff[k + 1] - soff[k]) * int(off[k + 1] - off[k]) for k in range(B)]
    counts, choices, rc = sentinel(nh, np.int32), sentinel(nh, np.int32), sentinel(nh + B, np.int32)
    models, tcws = sentinel(nh * 12, np.float64).reshape(nh, 12), sentinel(nh * 16, np.float32).reshape(nh, 4, 4)
    flags, inl, best, infos = sentinel(sum(nfl), np.uint8), sentinel(np_, np.uint8), sentinel(np_, np.uint8), sentinel(B, R.INFO_DTYPE)
    p = lambda a: a.ctypes.data   # noqa: E731
    assert pkg.matcher_lib().orbp_pnp_ransac_batch(p(b["corrs"]), p(off) + 4, B - 1, p(b["problems"]) + b["problems"].itemsize, p(sets), p(soff) + 4,
                                                   p(b["prior"]), p(counts), p(models), p(tcws), p(choices), p(flags), p(rc), p(inl), p(best),
                                                   p(infos), 0) == pkg.ORBX_OK
    for a, first in ((counts, h0), (choices, h0), (models, h0), (tcws, h0), (rc, h0), (inl, p0), (best, p0)):
        assert untouched(a[:first])                                # problem 0's ranges
    singles = {1: None, 2: run(pkg, S.BATCH_3[1]), 3: run(pkg, S.BATCH_3[2])}
    fb = 0
    for k in range(1, B):
        c = k - 1                                                  # the problem's number in this call
        h, q = slice(soff[k], soff[k + 1]), slice(off[k], off[k + 1])
        r = slice(soff[k] + c, soff[k + 1] + c + 1)                # refined_counts: set_offsets[b] + b, b counted in THIS call
        o = singles[k]
        if o is None:                                              # the empty problem
            assert (infos[c]["n"], infos[c]["iterations"], infos[c]["no_more"], infos[c]["pose"]) == (0, 0, 1, 0) and list(rc[r]) == [-1]
            continue
        for name in R.INFO_DTYPE.names:
            assert np.asarray(infos[c][name]).tobytes() == np.asarray(o[name], R.INFO_DTYPE[name].base).tobytes(), (k, name)
        assert (inl[q] == o["inliers"]).all() and (best[q] == o["best_flags"]).all() and (rc[r] == o["refined_counts"]).all()
        assert counts[h].tobytes() == o["counts"].tobytes() and choices[h].tobytes() == o["choices"].tobytes()
        assert models[h].tobytes() == o["models"].tobytes() and tcws[h].tobytes() == o["tcws"].tobytes()
        assert flags[fb:fb + nfl[k]].tobytes() == o["flags"].tobytes()                  # flags start at flags[0]
        fb += nfl[k]
    assert fb == sum(nfl[1:]) and untouched(flags[fb:]) and untouched(infos[B - 1:])
    assert untouched(rc[h0 + (nh - h0) + B - 1:]) and not untouched(rc[h0:h0 + (nh - h0) + B - 1])


def test_two_calls_through_the_c_abi(pkg):
    """the state carried by the caller: the first call's best flags, best count and iterations run go into the second call, in which
    a qualifying iteration that is no record returns the refinement of the PRIOR set"""
    L = pkg.matcher_lib()
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    sc = S.case("hit_60")
    n, sets = len(sc["corrs"]), np.ascontiguousarray(sc["sets"], np.int32)
    prob = S.problem(sc)

    def abi(prob, sets, prior):
        its = len(sets)
        counts, rc = np.zeros(its, np.int32), np.zeros(its + 1, np.int32)
        inl, best, info = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(1, R.INFO_DTYPE)
        assert L.orbp_pnp_ransac(p(sc["corrs"]), n, p(prob), p(sets), its, p(prior), p(counts), None, None, None, None, p(rc), p(inl), p(best),
                                 p(info), 0) == pkg.ORBX_OK
        return counts, rc, inl, best, info[0]
    c1, rc1, inl1, best1, i1 = abi(prob, sets, None)
    r1 = S.reference("hit_60")
    assert i1["hit_iteration"] == r1["hit_iteration"] >= 0 and (best1 == r1["best_flags"]).all() and (inl1 == r1["inliers"]).all()
    sc2, r2 = S.case("two_calls"), S.reference("two_calls")
    prob2 = prob.copy()
    prob2["iterations_done"], prob2["prior_best_inliers"] = i1["iterations_run"], i1["best_inliers"]
    assert prob2.tobytes() == S.problem(sc2).tobytes()
    c2, rc2, inl2, best2, i2 = abi(prob2, np.ascontiguousarray(sc2["sets"], np.int32), best1)
    assert i2["pose"] == R.POSE_REFINED and i2["best_iteration"] == -1 and i2["hit_iteration"] == r2["hit_iteration"] > 0
    assert c2[i2["hit_iteration"]] <= i1["best_inliers"] and c2[i2["hit_iteration"]] >= sc["min_inliers"]
    assert rc2[len(c2)] == r2["rcounts"][-1] == i2["refined_inliers"] and (rc2[:-1] == -1).all()
    assert (inl2 == r2["inliers"]).all() and (best2 == best1).all() and S.same(i2["Tcw"].reshape(4, 4), r2["Tcw"])
    assert S.same(i2["Tcw"].reshape(4, 4), i1["Tcw"].reshape(4, 4))              # the same set refined again: the same pose


def test_three_host_threads_at_once(pkg):
    names = ("hit_60", "n_1100", "two_calls")
    got, barrier = {}, threading.Barrier(3)

    def worker(name):
        barrier.wait()
        got[name] = [call(pkg, S.case(name)) for _ in range(2)]
        got[name + "/rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
    ts = [threading.Thread(target=worker, args=(k,)) for k in names]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    for k in names:
        assert got[k + "/rc"] == pkg.ORBX_OK and all(same_bytes(o, run(pkg, k)) for o in got[k]), k


def test_release_scratch_then_call(pkg):
    first = run(pkg, "wave_65")
    assert pkg.matcher_lib().orbx_thread_release_scratch() == pkg.ORBX_OK
    assert same_bytes(call(pkg, S.case("wave_65")), first)


def test_argument_errors_launch_nothing(pkg):
    """every ORBX_ERR_ARG case returns before the device is touched: after orbx_thread_release_scratch the thread holds no stream
    and no scratch, and a refused call leaves the outputs as they were"""
    L = pkg.matcher_lib()
    assert L.orbx_thread_release_scratch() == pkg.ORBX_OK
    sc = S.case("hit_60")
    n, sets = len(sc["corrs"]), np.ascontiguousarray(sc["sets"][:8], np.int32)
    for kw in bad_calls(pkg, sc, sets):
        counts = np.full(8, -7, np.int32)
        kw = dict(kw)
        assert abi_call(pkg, sc, kw.pop("sets", sets), counts, **kw) == pkg.ORBX_ERR_ARG, kw
        assert (counts == -7).all()
    counts = np.full(8, -7, np.int32)
    assert abi_call(pkg, sc, sets, counts) == pkg.ORBX_OK and (counts == S.reference("hit_60")["counts"][:8]).all()


def abi_call(pkg, sc, sets, counts, corrs=None, n=None, prob=None, its=None, prior=None, null=()):
    p = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    corrs = sc["corrs"] if corrs is None else corrs
    n = len(sc["corrs"]) if n is None else n
    prob = S.problem(sc) if prob is None else prob
    its = len(sets) if its is None else its
    inl, best, info = np.zeros(len(sc["corrs"]), np.uint8), np.zeros(len(sc["corrs"]), np.uint8), np.zeros(1, R.INFO_DTYPE)
    a = dict(corrs=corrs, prob=prob, sets=sets, counts=counts, inl=inl, best=best, info=info)
    for k in null:
        a[k] = None
    return pkg.matcher_lib().orbp_pnp_ransac(p(a["corrs"]), n, p(a["prob"]), p(a["sets"]), its, p(prior), p(a["counts"]), None, None, None, None,
                                             None, p(a["inl"]), p(a["best"]), p(a["info"]), 0)


def bad_calls(pkg, sc, sets):
    n = len(sc["corrs"])
    out = [dict(null=(k,)) for k in ("corrs", "prob", "sets", "counts", "inl", "best", "info")] + [dict(n=-1), dict(its=-1), dict(n=3)]
    bad = sets.copy(); bad[5, 1] = n; out.append(dict(sets=bad))                  # an index out of range
    bad = sets.copy(); bad[0, 0] = -1; out.append(dict(sets=bad))
    bad = sets.copy(); bad[3, 3] = bad[3, 0]; out.append(dict(sets=bad))          # a set naming a correspondence twice
    for v in (-1.0, np.nan, np.inf):
        c = sc["corrs"].copy(); c["sigma2"][7] = v; out.append(dict(corrs=c))
    pr = S.problem(sc); pr["prior_best_inliers"] = 3; out.append(dict(prob=pr))   # a prior count without prior flags
    fl = np.zeros(n, np.uint8); fl[:5] = 1; out.append(dict(prob=pr, prior=fl))   # 3 != 5
    pr = S.problem(sc); pr["min_inliers"] = n + 1; out.append(dict(prob=pr))      # sets for a problem with n < min_inliers
    return out


def test_python_solver_iterates_as_the_reference(pkg):
    """PnPsolver.iterate(5) on a fresh solver runs ALL max_iterations (the loop's ||), hits as the restatement does, and carries its
    state into a second call; a solver with fewer correspondences than min_inliers answers no_more without a device call"""
    sc, r = S.case("hit_60"), S.reference("hit_60")
    so = pkg.PnPsolver(sc["corrs"], sc["K"])
    so.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
    assert (so.min_inliers, so.max_iterations, so.planned(5)) == (30, 35, 35)
    T, nm, inl, n = so.iterate(5, sc["sets"])
    assert T is not None and not nm and n == r["refined_inliers"] and (inl == r["inliers"]).all() and S.same(T, r["Tcw"])
    assert so.iterations == r["iterations_run"] and so.best_inliers == r["best_inliers"] and so.planned(5) == 35 - so.iterations
    sc2, r2 = S.case("two_calls"), S.reference("two_calls")
    T2, nm2, inl2, n2 = so.iterate(so.max_iterations, sc2["sets"])
    assert S.same(T2, r2["Tcw"]) and n2 == r2["refined_inliers"] and so.iterations == r["iterations_run"] + r2["iterations_run"]
    sc = S.case("n_9")
    so = pkg.PnPsolver(sc["corrs"], sc["K"])
    so.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
    T, nm, inl, n = so.iterate(5)
    assert T is None and nm and n == 0 and len(inl) == 9 and not inl.any() and so.planned(5) == 0
    sc, r = S.case("exhausted_60"), S.reference("exhausted_60")
    so = pkg.PnPsolver(sc["corrs"], sc["K"])
    so.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
    T, nm, inl, n = so.find(sc["sets"])
    assert nm and n == 30 and S.same(T, r["best_Tcw"]) and (inl == r["best_flags"]).all()


def test_iterate_all_equals_separate_solvers(pkg):
    names = ("hit_60", "n_9", "wave_65", "exhausted_60")

    def solvers():
        out = []
        for k in names:
            so = pkg.PnPsolver(S.case(k)["corrs"], S.case(k)["K"])
            so.set_ransac_parameters(0.99, 10, 300, 4, 0.5, 5.991)
            out.append(so)
        return out
    a, b = solvers(), solvers()
    sets = [np.tile(S.case(k)["sets"], (3, 1)) for k in names]              # wave_65 has 12 sets, a fresh call takes 35
    ra = pkg.PnPsolver.iterate_all(a, 5, sets)
    for sb, s, x in zip(b, sets, ra):
        y = sb.iterate(5, s)
        assert (x[0] is None) == (y[0] is None) and x[1] == y[1] and x[3] == y[3] and (x[2] == y[2]).all()
        assert x[0] is None or x[0].tobytes() == y[0].tobytes()
    assert ra[1][:2] == (None, True) and ra[0][0] is not None
