"""GPU: the k_eg_* kernels and their host driver (orbg_optimize_essential_graph, csrc/orbx_essential.hip) against the numpy restatement
tests/essential_ref.py, at the shapes of tests/essential_scene.py: CASES.  The way the loop ended equal; free vertices, factor blocks
and levels equal; the double estimates within 64 x S, where S is the deviation the restatement itself shows over 16 draws of (the
order of its sums over edges and vertices, sin / cos / acos / log / exp moved by +-2 ulp) - the kernels differ from it by the order
of their chi2 and computeScale sums and by the device's elementary functions; the float outputs within 1 ulp + 64 x S; the trials of
every iteration whose min |rho| exceeds 1e-6 equal, and the totals where every iteration's does (at or below it the sign of rho is
rounding noise, and how many such iterations follow differs between the restatement's own draws); two runs byte-identical; iterations = 1;
ten rejected trials leave nothing behind (iterations = 2 against 3); argument
errors; empty problems; a second host thread before and after orbx_thread_release_scratch; fresh scratch filled.

The numeric Jacobian divides rounding noise by 2e-9, so S is near 1e-7 where a residual remains at the optimum, and near 1e-14 where
the graph is a tree and every residual goes to zero.

Every device array is written before it is read: est[0], est[1], meas by k_eg_init; err, partChi by k_eg_edges; jac by
k_eg_edges<true> for the sides that k_eg_vertex / k_eg_offdiag read (the side of a fixed vertex is neither written nor read); Hd, b,
Hoff by k_eg_vertex / k_eg_offdiag; L, x, rec.ok by k_eg_assemble; partScale by k_eg_update; rec.linChi / tmpChi / scale by
k_eg_reduce before the host's copy.  Never read: the upper triangle of a diagonal factor block, rec.pad, EgDev.pad.

Measured on one MI355X (S from the restatement alone; the difference is max |kernels - restatement| over every double estimate - q,
t, s of every vertex; end and trials are kernels / restatement, trials per iteration; every case gave the same bytes twice):
    case                 S          difference           end      trials                            blocks levels launches
    chain                3.020e-14  0.000e+00  0.00 S    1 / 1    1 1 1 10   / 1 1 1 10               21     11      499
    ring_fixed_scale     5.965e-07  2.436e-07  0.41 S    1 / 1    1 1 1 10   / 1 1 1 10              123     23      967
    ring_free_scale      1.780e-06  0.000e+00  0.00 S    1 / 1    1 10       / 1 10                  123     23      813
    clique               2.665e-15  8.882e-16  0.33 S    1 / 1    1 1 1 10   / 1 1 1 1 10             15      5      265
    two_branches         7.994e-15  0.000e+00  0.00 S    1 / 1    1 1 1 10   / 1 1 1 10               18      5      265
    fixed_mid            2.007e-13  0.000e+00  0.00 S    1 / 1    1 1 1 1 10 / 1 1 1 1 10             28     11      540
    dup_pair             2.398e-14  0.000e+00  0.00 S    1 / 1    1 1 1 10   / 1 1 1 10               13      7      343
    kinds                6.951e-07  0.000e+00  0.00 S    1 / 1    1 1 1 1 10 / 1 1 1 1 10             24      9      456
    wide                 1.446e-07  0.000e+00  0.00 S    1 / 1    1 1 1 10   / 1 1 1 10              532     79     3151
    branches             6.376e-06  1.387e-09  0.00 S    1 / 1    1 10       / 1 10                   25      9      351
    ring_nbad            4.319e-06  2.159e-06  0.50 S    4 / 4    1 1 1 1 1  / 1 1 1 1 1             123     23      387
    ring_rejected        3.452e-04  2.039e-04  0.59 S    1 / 1    1 1 10     / 1 1 10                123     23      890
    ring_fixed_scale, 1  5.965e-07  0.000e+00  0.00 S    0 / 0    1          / 1                     123     23       79
    ring_free_scale, 1   1.780e-06  0.000e+00  0.00 S    0 / 0    1          / 1                     123     23       79
    ring_rejected, 2     4.151e-04  2.039e-04  0.49 S    0 / 0    1 1        / 1 1                   123     23      156
(`, 1`, `, 2`: iterations = 1, 2.  end 1: ten rejected trials, 0: the iterations asked for, 4: three iterations of negligible gain.)
ring_rejected does not converge (its second accepted step has rho = 0.86 and ten rejected trials follow, rho from -1.2 to -0.23),
so its S is large and 64 x S says little; the call with iterations = 3 returned the bytes of the call with iterations = 2 in est,
Tcw and the points, and an info that differs in iterations, trials, trials_it, end and launches alone.  The float outputs differ from the restatement's
in their last place at most.  The iterations whose min |rho| is at or below 1e-6 are not compared in their counts: clique's fourth
(1.7e-27), where the kernels reject and the restatement accepts once more; from the second or third iteration on every
fixed-scale case is there.  Where a residual remains at the optimum the way a converged call ends is decided by the sign of such a
rho: the restatement's own draws end by ten rejected trials or by three iterations of negligible gain on ring_fixed_scale-like
scenes (seeds were chosen where most draws agree with the restatement), and the kernels' ending is asserted against the restatement's."""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import essential_ref as R        # noqa: E402
import essential_scene as S      # noqa: E402
from test_scratch_fill_gpu import PAIR_BLOCKS, fill      # noqa: E402,F401   the fixture that fills every fresh scratch block

pytestmark = pytest.mark.gpu
MARGIN = S.MARGIN


def call(pkg, sc, **kw):
    return pkg.optimize_essential_graph(sc["vertices"], sc["edges"], sc["points"], sc["fix_scale"], **kw)


def as_bytes(res):
    T, X, est, info = res
    return (T.tobytes(), X.tobytes(), est.tobytes(), tuple(sorted((k, str(v)) for k, v in info.items())))


def compare(name, res, ref, dev):
    """the comparison of the module's docstring; ref: the restatement's result, dev: S"""
    T, X, est, info = res
    for what, m in ref["trace"].margin.items():      # asserted per draw in tests/test_essential_cpu.py
        assert m > MARGIN, "scene %s: %s at its threshold - choose another seed" % (name, what)
    ri = ref["info"]
    minrho = [min(abs(x) for x in it["rho"]) for it in ref["trace"].iterations]
    diff = float(np.abs(est - ref["est"]).max()) if len(est) else 0.0
    print("%s: S = %.3e, kernels - restatement = %.3e (%.2f S); end %d / %d, iterations %d / %d, trials %s / %s (kernels / restatement), "
          "min |rho| %s, blocks %d, levels %d, launches %d" % (
              name, dev, diff, diff / dev if dev else 0.0, info["end"], ri["end"], info["iterations"], ri["iterations"],
              info["trials_it"][:info["iterations"]], ri["trials_it"][:ri["iterations"]], ["%.1e" % r for r in minrho], info["blocks"],
              info["levels"], info["launches"]))
    for k in ("free_vertices", "blocks", "levels"):
        assert info[k] == ri[k], (k, info[k], ri[k])
    assert info["end"] == ri["end"], (info["end"], ri["end"])
    assert diff <= 64 * dev, (diff, dev)
    for a, b in ((T, ref["Tcw"]), (X, ref["pts"])):
        ulp = np.spacing(np.maximum(np.float32(1), np.abs(b)).astype(np.float32)).astype(np.float64)
        assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulp + 64 * dev).all()
    for k, r in enumerate(minrho):
        if r > 1e-6:      # at or below it the sign of rho is rounding noise
            assert info["iterations"] > k and info["trials_it"][k] == ri["trials_it"][k], (k, info["trials_it"][:8], ri["trials_it"][:8])
    if all(r > 1e-6 for r in minrho):
        assert info["iterations"] == ri["iterations"] and info["trials"] == ri["trials"]
    rel = abs(info["chi2_first"] - ri["chi2_first"])
    assert rel <= 64 * dev * max(1.0, ri["chi2_first"]) + 1e-12 * ri["chi2_first"]


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernels_against_restatement(pkg, name):
    sc, ref, draws, dev = S.reference(name)
    res = call(pkg, sc)
    compare(name, res, ref, dev)
    assert as_bytes(res) == as_bytes(call(pkg, sc))                              # determinism: identical bytes in all outputs
    fixed = sc["vertices"]["fixed"] != 0
    want = sc["vertices"]["Scw"][fixed]
    assert res[2][fixed].tobytes() == np.concatenate([want["q"], want["t"], want["s"][:, None]], 1).tobytes()      # a fixed vertex keeps its estimate


@pytest.mark.parametrize("name", ["ring_fixed_scale", "ring_free_scale"])
def test_one_iteration(pkg, name):
    sc, _, _, dev = S.reference(name)
    ref = S.run(sc, iterations=1)
    res = call(pkg, sc, iterations=1)
    assert res[3]["iterations"] == 1
    compare(name + ", one iteration", res, ref, dev)


def test_ten_popped_trials_leave_nothing_behind(pkg):
    """ring_rejected runs [1, 1, 10]: its third iteration is ten rejected trials (rho from -1.2 to -0.23), each of them popped.  So
    the call with iterations=3 must return the bytes of the call with iterations=2 in est, Tcw and the points, and an info that
    differs in iterations, trials, trials_it, end and launches alone - a check that needs no tolerance, where 64 x S = 0.02 of the
    full comparison says little.  The call cut short is compared with the restatement cut short, S being that run's own spread."""
    sc, ref2, _, dev2 = S.reference_cut("ring_rejected", 2)
    r2, r3 = call(pkg, sc, iterations=2), call(pkg, sc, iterations=3)
    i2, i3 = r2[3], r3[3]
    assert (i2["iterations"], i2["end"], list(i2["trials_it"][:3])) == (2, R.END_ITERATIONS, [1, 1, 0])
    assert (i3["iterations"], i3["end"], list(i3["trials_it"][:3])) == (3, R.END_QMAX, [1, 1, 10])
    assert r2[2].tobytes() == r3[2].tobytes() and r2[0].tobytes() == r3[0].tobytes() and r2[1].tobytes() == r3[1].tobytes()
    assert {k for k in i2 if str(i2[k]) != str(i3[k])} == {"iterations", "trials", "trials_it", "end", "launches"}
    compare("ring_rejected, 2 iterations", r2, ref2, dev2)
    ref3 = S.reference("ring_rejected")[1]
    assert ref3["info"]["iterations"] == 3 and ref3["est"].tobytes() == ref2["est"].tobytes()      # the restatement's two calls agree the same way


def test_empty_and_edgeless_problems(pkg):
    sc = S.case("chain")
    e = dict(sc, vertices=sc["vertices"][:0], edges=sc["edges"][:0], points=sc["points"][:0])
    T, X, est, info = call(pkg, e)
    assert len(T) == 0 and len(X) == 0 and info["iterations"] == 0 and info["launches"] == 0
    for variant in (dict(sc, edges=sc["edges"][:0]), dict(sc, points=sc["points"][:0])):
        ref = S.run(variant)
        T, X, est, info = call(pkg, variant)
        assert info["iterations"] == ref["info"]["iterations"] and info["free_vertices"] == ref["info"]["free_vertices"]
        if len(variant["edges"]) == 0:      # E == 0: nothing is optimised, every output is the conversion of the input
            assert info == ref["info"] and est.tobytes() == ref["est"].tobytes() and T.tobytes() == ref["Tcw"].tobytes() and X.tobytes() == ref["pts"].tobytes()


def test_argument_errors_do_not_touch_the_device(pkg):
    L = pkg.matcher_lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    sc = S.case("chain")
    vt, ed, pt = sc["vertices"].copy(), sc["edges"].copy(), sc["points"].copy()
    N, E, P = len(vt), len(ed), len(pt)
    To, Po = np.full((N, 16), 7, np.float32), np.full((P, 3), 7, np.float32)
    f = L.orbg_optimize_essential_graph
    # device 99 does not exist: a call that got as far as the device would say so instead
    bad = ed.copy(); bad["j"][2] = bad["i"][2]
    assert f(p(vt), N, p(bad), E, p(pt), P, 1, 20, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    bad = ed.copy(); bad["i"][0] = N
    assert f(p(vt), N, p(bad), E, p(pt), P, 1, 20, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    bad = ed.copy(); bad["kind"][0] = 2
    assert f(p(vt), N, p(bad), E, p(pt), P, 1, 20, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    bv = vt.copy(); bv["Scw"]["t"][3, 1] = np.nan
    assert f(p(bv), N, p(ed), E, p(pt), P, 1, 20, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    bv = vt.copy(); bv["Scw"]["s"][1] = 0.0
    assert f(p(bv), N, p(ed), E, p(pt), P, 1, 20, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    bp = pt.copy(); bp["ref"][0] = -1
    assert f(p(vt), N, p(ed), E, p(bp), P, 1, 20, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    assert f(p(vt), N, p(ed), E, p(pt), P, 1, pkg.EG_MAX_ITERATIONS + 1, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    assert f(p(vt), N, p(ed), E, p(pt), P, 1, 20, None, p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    assert f(p(vt), N, None, E, p(pt), P, 1, 20, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_ARG
    assert f(p(vt), N, p(ed), E, p(pt), P, 1, 20, p(To), p(Po), None, None, 99) == pkg.ORBX_ERR_NO_DEVICE
    assert (To == 7).all() and (Po == 7).all()


def test_second_host_thread_before_and_after_release(pkg):
    """scratch is per host thread: another thread gets the same bytes, releases its scratch, and gets them again"""
    sc = S.case("kinds")
    here = as_bytes(call(pkg, sc))
    got = {}

    def worker():
        try:
            got["first"] = as_bytes(call(pkg, sc))
            got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
            got["after"] = as_bytes(call(pkg, sc))
            got["rc2"] = pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001
            got["error"] = e
    th = threading.Thread(target=worker)
    th.start(); th.join()
    assert "error" not in got, got.get("error")
    assert got["first"] == got["after"] == here and got["rc"] == got["rc2"] == pkg.ORBX_OK
    assert as_bytes(call(pkg, sc)) == here


@pytest.mark.parametrize("name", ["ring_free_scale", "two_branches"])
def test_results_do_not_depend_on_fresh_scratch(pkg, fill, name):      # noqa: F811
    sc, ref, _, dev = S.reference(name)

    def run():
        res = call(pkg, sc)
        return {"bytes": dict(enumerate(as_bytes(res))), "res": res}
    fill.three(run, PAIR_BLOCKS, lambda raw: compare(name, raw["res"], ref, dev), "essential graph " + name)
