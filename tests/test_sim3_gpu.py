"""GPU: k_sim3_prepare / k_sim3_ransac / k_sim3_select (orbs_*, csrc/orbx_sim3.hip) against the numpy restatement tests/sim3_ref.py on
every scene of tests/sim3_scene.py.

What is not bit-determined on the device.  With -ffp-contract=off, correctly rounded float and double + - * / sqrt, integer counts
(ballot + popcount) and no value crossing lanes, the only operations whose result may differ from the restatement's are the
double atan2, sin and cos of one hypothesis (the C library's on the host, the device math library's on the GPU).  ROCm's
documentation as installed states no ulp bound for them, so the effect was measured with 2 ulp: the restatement was rerun with the
three results moved by +-2 ulp in all 8 sign combinations on every scene (sim3_scene.margins).  Measured: the largest deviation
of any entry of s, R, t, T12 is 0 on every scene, and the largest relative change of any err1 / err2 below 4 x its threshold is
0 - the three doubles feed `vec = (float)(vec * 2 ang / |vec|)` and `R = (float)(...)`, and a change of 4e-16 relative moves a
float result only when it lies within 7e-9 of a rounding boundary, which none of the 1 106 hypotheses x 12 values here does.
So the float tolerance (4 x the largest deviation, per scene) is 0: byte equality, a NaN equal to a NaN; and an evaluation is
borderline (within 4 x 0 of its threshold) only when an error EQUALS its threshold, which happens nowhere: the borderline set
is empty on every scene (0 of 74 413 evaluations, against the 0.5 % allowed).  The test keeps the general form - tolerance and
borderline set come from sim3_scene.margins / borderline at run time - so a scene added later is held to its own measurement.

Conditions, asserted on the restatement alone (sim3_scene.assert_conditions; tests/test_sim3_cpu.py has no GPU and the seeds were
chosen there): borderline evaluations are at most 0.5 % of a scene's; at the hit iteration the count exceeds min_inliers by more
than that iteration's borderline count; no earlier iteration is within its borderline count of min_inliers."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
_runs = {}


def run(pkg, name):
    """one single call per scene, shared by the tests"""
    if name not in _runs:
        sc = S.case(name)
        _runs[name] = pkg.sim3_ransac_batch(sc["pairs"], [0, len(sc["pairs"])], S.problem(sc), sc["sets"], [0, len(sc["sets"])])[0]
    return _runs[name]


def same_bytes(a, b):
    keys = ("counts", "models", "flags", "hit_inliers", "n", "iterations", "hit_iteration", "best_iteration", "best_inliers", "s", "R", "t", "T12")
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)


def close(a, b, tol):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if tol == 0:
        return S.same_floats(a, b)
    nan = np.isnan(a) | np.isnan(b)
    return bool((np.isnan(a) == np.isnan(b)).all() and (np.abs(a.astype(np.float64) - b)[~nan] <= tol).all())


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernels_equal_the_restatement(pkg, name):
    dm, de = S.margins(name)
    tol, rel = 4 * dm, 4 * de
    sc, r, bl = S.assert_conditions(name, rel)
    nb = bl.sum(axis=1)
    o = run(pkg, name)
    assert (o["n"], o["iterations"]) == (r["n"], r["iterations"])
    assert o["flags"].shape == r["flags"].shape and ((o["flags"] == r["flags"]) | bl).all()             # equal outside the borderline set
    assert (np.abs(o["counts"].astype(np.int64) - r["counts"]) <= nb).all()                              # up to each iteration's borderline count
    assert o["hit_iteration"] == r["hit_iteration"]
    h = r["hit_iteration"]
    if h >= 0:
        assert abs(o["best_inliers"] - r["best_inliers"]) <= nb[h] and ((o["hit_inliers"] == r["hit_inliers"]) | bl[h]).all()
        assert o["best_iteration"] == h
    else:
        assert not o["hit_inliers"].any()
        if r["iterations"]:
            assert abs(o["best_inliers"] - r["best_inliers"]) <= nb.max()
        if not nb.any():
            assert o["best_iteration"] == r["best_iteration"] and o["best_inliers"] == r["best_inliers"]
    assert close(o["models"], r["models"], tol)
    if o["best_iteration"] == r["best_iteration"]:
        assert close(o["s"], r["s"], tol) and close(o["R"], r["R"], tol) and close(o["t"], r["t"], tol) and close(o["T12"], r["best_T12"], tol)
    print("%s: tolerance %g, %d borderline of %d; hit %d, best %d with %d" % (name, tol, bl.sum(), bl.size, o["hit_iteration"], o["best_iteration"],
                                                                               o["best_inliers"]))


def test_degenerate_terminates_with_nothing_counted(pkg):
    o = run(pkg, "degenerate")
    assert not o["counts"].any() and not o["flags"].any() and not o["hit_inliers"].any()
    assert (np.isfinite(o["models"]) | np.isnan(o["models"])).all() and np.isnan(o["models"][:, 1:]).all()
    assert (o["hit_iteration"], o["best_iteration"], o["best_inliers"]) == (-1, 3, 0)


def test_two_runs_give_the_same_bytes(pkg):
    for name in ("hit_60_scale", "n_257", "degenerate"):
        sc = S.case(name)
        again = pkg.sim3_ransac_batch(sc["pairs"], [0, len(sc["pairs"])], S.problem(sc), sc["sets"], [0, len(sc["sets"])])[0]
        assert same_bytes(again, run(pkg, name)), name


def test_batch_equals_the_single_calls(pkg):
    b = S.batch(S.BATCH_3)
    outs = pkg.sim3_ransac_batch(b["pairs"], b["offsets"], b["problems"], b["sets"], b["set_offsets"])
    assert len(outs) == 4
    e = outs[1]                                                    # the empty problem
    assert (e["n"], e["iterations"], e["hit_iteration"], e["best_iteration"], e["best_inliers"]) == (0, 0, -1, -1, 0) and not e["T12"].any()
    for o, name in zip([outs[0]] + outs[2:], S.BATCH_3):
        assert same_bytes(o, run(pkg, name)), name
    assert outs[2]["iterations"] == 0 and outs[2]["n"] == 19 and outs[2]["hit_iteration"] == -1      # n_19: pairs but no iteration


def test_batch_whose_first_offset_is_not_zero(pkg):
    """the C ABI called on problems 1 .. of the four-problem batch: offsets + 1, set_offsets + 1, problems + 1, B - 1, the arrays'
    base pointers as in the full call.  Then offsets[0] = 60 and set_offsets[0] > 0 (p0, h0 of csrc/orbx_sim3.hip).  counts, models
    and hit_inliers land where the full call puts them and equal the single calls'; flags and infos are counted from this call's
    first problem; no byte of problem 0's ranges and none behind the used ranges is written"""
    b = S.batch(S.BATCH_3)
    off, soff, B = b["offsets"], b["set_offsets"], len(b["problems"])
    p0, h0, np_, nh = int(off[1]), int(soff[1]), int(off[B]), int(soff[B])
    assert B == 4 and p0 == 60 and h0 > 0 and nh > h0
    sets = np.ascontiguousarray(b["sets"], np.int32)
    nfl = [int(soff[k + 1] - soff[k]) * int(off[k + 1] - off[k]) for k in range(B)]
    sentinel = lambda count, dtype: np.full(count * np.dtype(dtype).itemsize, 0xA5, np.uint8).view(dtype)   # noqa: E731
    untouched = lambda a: bool((np.ascontiguousarray(a).view(np.uint8) == 0xA5).all())                        # noqa: E731
    counts, models = sentinel(nh, np.int32), sentinel(nh * 13, np.float32).reshape(nh, 13)
    flags, hit, infos = sentinel(sum(nfl), np.uint8), sentinel(np_, np.uint8), sentinel(B, S.INFO_DTYPE)
    p = lambda a: a.ctypes.data   # noqa: E731
    assert pkg.matcher_lib().orbs_sim3_ransac_batch(p(b["pairs"]), p(off) + 4, B - 1, p(b["problems"]) + b["problems"].itemsize, p(sets), p(soff) + 4,
                                                    p(counts), p(models), p(flags), p(hit), p(infos), 0) == pkg.ORBX_OK
    assert untouched(counts[:h0]) and untouched(models[:h0]) and untouched(hit[:p0])                        # problem 0's ranges
    singles = {1: None, 2: run(pkg, S.BATCH_3[1]), 3: run(pkg, S.BATCH_3[2])}
    fb = 0
    for k in range(1, B):
        c = k - 1                                                  # the problem's number in this call
        h, q = slice(soff[k], soff[k + 1]), slice(off[k], off[k + 1])
        o = singles[k]
        if o is None:                                              # the empty problem
            assert (infos[c]["n"], infos[c]["iterations"], infos[c]["hit_iteration"], infos[c]["best_iteration"]) == (0, 0, -1, -1)
            continue
        for name in S.INFO_DTYPE.names:
            assert np.asarray(infos[c][name]).tobytes() == np.asarray(o[name], S.INFO_DTYPE[name].base).tobytes(), (k, name)
        assert (hit[q] == o["hit_inliers"]).all() and counts[h].tobytes() == o["counts"].tobytes() and models[h].tobytes() == o["models"].tobytes()
        assert flags[fb:fb + nfl[k]].tobytes() == o["flags"].tobytes()                  # flags start at flags[0]
        fb += nfl[k]
    assert fb == sum(nfl[1:]) and untouched(flags[fb:]) and untouched(infos[B - 1:])


def test_python_solver_chunks_as_the_restatement(pkg):
    import sim3_ref as R
    for name in ("hit_60", "exhausted_60", "n_19"):
        sc, r = S.case(name), S.reference(name)
        so = pkg.Sim3Solver(sc["pairs"], sc["Tcw1"], sc["Tcw2"], sc["K1"], sc["K2"], sc["fix_scale"])
        so.set_ransac_parameters(0.99, sc["min_inliers"], 300)
        sets = sc["sets"][:so.max_iterations]
        tr = R.ransac(sc["pairs"], sc["Tcw1"], sc["Tcw2"], sc["K1"], sc["K2"], sc["fix_scale"], sc["min_inliers"], sets)
        ref = R.Solver(tr, sc["min_inliers"])
        for _ in range(70):
            T, nm, inl, n = so.iterate(5, sets)
            Tr, nmr, inlr, nr = ref.iterate(5)
            assert (T is None) == (Tr is None) and nm == nmr and n == nr and (inl == inlr).all() and so.iterations == ref.it
            assert T is None or S.same_floats(T, Tr)
            if nm:
                break
        assert nm and so.best_iteration == ref.best


def test_iterate_all_equals_separate_solvers(pkg):
    names = ("hit_60", "n_19", "wave_65")
    def solvers():
        out = []
        for k in names:
            sc = S.case(k)
            so = pkg.Sim3Solver(sc["pairs"], sc["Tcw1"], sc["Tcw2"], sc["K1"], sc["K2"], sc["fix_scale"])
            so.set_ransac_parameters(0.99, sc["min_inliers"], 300)
            out.append(so)
        return out
    a, b = solvers(), solvers()
    sets = [S.case(k)["sets"] for k in names]
    pkg.Sim3Solver.iterate_all(a, sets)
    assert a[1]._trace is None and a[0]._trace is not None
    for sa, sb, s in zip(a, b, sets):
        ra, rb = sa.find(), sb.find(s)
        assert (ra[0] is None) == (rb[0] is None) and ra[1:2] == rb[1:2] and ra[3] == rb[3] and (ra[2] == rb[2]).all()
        assert ra[0] is None or ra[0].tobytes() == rb[0].tobytes()


def test_second_host_thread_after_release(pkg):
    """a second host thread builds its own scratch, mirror and stream and gets the first thread's bytes; the first, after
    orbx_thread_release_scratch, builds them again and gets them too"""
    sc = S.case("wave_65")
    call = lambda: pkg.sim3_ransac_batch(sc["pairs"], [0, 65], S.problem(sc), sc["sets"], [0, len(sc["sets"])])[0]   # noqa: E731
    first = call()
    assert pkg.matcher_lib().orbx_thread_release_scratch() == pkg.ORBX_OK
    got = {}

    def worker():
        got["r"] = call()
        got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert got["rc"] == pkg.ORBX_OK and same_bytes(got["r"], first) and same_bytes(call(), first) and same_bytes(first, run(pkg, "wave_65"))


def test_scratch_regrows_inside_one_thread(pkg):
    """a fresh host thread: a small scene reserves the staging pair at its 1 MiB floor, a batch of K copies of n_257 whose flag
    bytes alone exceed that floor makes it regrow, the small scene runs in the regrown pair; every output equals the single calls'"""
    big = S.case("n_257")
    n, its = len(big["pairs"]), len(big["sets"])
    K = (1 << 20) // (its * n) + 1                                  # the smallest K with K * iterations * pairs > 1 MiB
    assert (K - 1) * its * n <= 1 << 20 < K * its * n
    small = S.case("wave_65")
    call_small = lambda: pkg.sim3_ransac_batch(small["pairs"], [0, 65], S.problem(small), small["sets"], [0, len(small["sets"])])[0]   # noqa: E731
    got = {}

    def worker():
        got["first"] = call_small()
        got["big"] = pkg.sim3_ransac_batch(np.tile(big["pairs"], K), np.arange(K + 1) * n, np.tile(S.problem(big), K),
                                           np.tile(big["sets"], (K, 1)), np.arange(K + 1) * its)
        got["again"] = call_small()
        got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
    t = threading.Thread(target=worker)
    t.start()
    t.join()
    assert len(got["big"]) == K and all(same_bytes(o, run(pkg, "n_257")) for o in got["big"])
    assert same_bytes(got["first"], run(pkg, "wave_65")) and same_bytes(got["again"], run(pkg, "wave_65"))
    assert got["rc"] == pkg.ORBX_OK
