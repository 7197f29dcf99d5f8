"""GPU: k_sim3_opt (orbz_optimize_sim3*, csrc/orbx_sim3opt.hip) against the numpy restatement tests/sim3opt_ref.py, at the shapes of
tests/sim3opt_scene.py: CASES.  Flags and counts equal; the double Sim3 within 64 x S, where S is the deviation the restatement
itself shows over 16 draws of (summation order, exp / sin / cos moved by +-2 ulp) - the kernel differs from it by its summation
order and by the device's exp / sin / cos; the float matrix within 1 ulp + 64 x S; two runs byte-identical; a batch equal to its
single calls, also when it outgrows the staging pair's floor on a fresh host thread; the rows past the LDS stage; the fixed scale;
the early return; independence of what fresh scratch held; argument errors.

Measured on one MI355X (S from the restatement alone; the difference is max |kernel - restatement| over q, t, s; iterations and
trials are kernel / restatement per round; S is large for doubles because g2o's numeric Jacobian divides rounding noise by 2e-9):
    case            S           difference        iterations       trials
    n0              0           0                 0 0 / 0 0        0 0 / 0 0
    n9              0           0                 5 0 / 5 0        9 0 / 9 0          (the input Sim3 goes out)
    n10             3.413e-07   1.096e-07 0.32 S  5 3 / 5 3        10 6 / 10 6
    clean64         5.012e-08   1.030e-08 0.21 S  5 3 / 5 2        5 16 / 5 11        (round 2: min |rho| = 0, not compared)
    out65           7.221e-08   2.224e-08 0.31 S  5 4 / 5 4        5 8 / 5 8
    fix_scale65     2.694e-08   1.448e-08 0.54 S  4 4 / 4 4        4 4 / 4 4
    drop_below10    0           0                 5 0 / 5 0        5 0 / 5 0          (the input Sim3 goes out)
    far             3.045e-08   1.296e-08 0.43 S  5 4 / 5 4        11 8 / 11 8
    nL              1.176e-07   4.182e-09 0.04 S  5 3 / 5 3        9 3 / 9 3
    nL+1            2.384e-07   9.777e-08 0.41 S  4 4 / 4 4        4 4 / 4 4
    n1.3L           9.512e-08   4.665e-08 0.49 S  5 4 / 5 4        5 4 / 5 4
    mixed300        8.760e-08   2.522e-08 0.29 S  4 4 / 4 4        4 4 / 4 4
The float matrices differ from the restatement's in their last place wherever the double estimates differ by 1e-8.
"""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sim3opt_ref as R        # noqa: E402
import sim3opt_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
MARGIN = S.MARGIN   # |chi2 / th2 - 1| below which a flag may differ (tests/test_poseopt_gpu.py's value)


def as_bytes(res):
    T, dr, ni, info = res
    return (T.tobytes(), dr.tobytes(), int(ni), info["correspondences"], info["bad"], info["rounds"], tuple(info["iterations"]),
            tuple(info["trials"]), info["q"].tobytes(), info["t"].tobytes(), np.float64(info["s"]).tobytes())


def check_against_reference(name, res):
    sc, ref, draws, dev = S.reference(name)
    T, dr, ni, info = res
    # the condition of the comparison (asserted per draw in tests/test_sim3opt_cpu.py): no live edge within the margin of th2
    for r, tr in enumerate(ref["trace"]):
        assert tr["min_margin"] > MARGIN, "scene %s: an edge is %.2e from th2 in round %d - choose another seed" % (name, tr["min_margin"], r)
    assert (ni, info["correspondences"], info["bad"], info["rounds"]) == (ref["ninliers"], ref["correspondences"], ref["bad"], ref["rounds"])
    assert (dr == ref["dropped"]).all()
    got = np.concatenate([info["q"], info["t"], [info["s"]]])
    diff = float(np.abs(got - ref["sim3"].vec()).max())
    ulp = np.spacing(np.maximum(np.float32(1), np.abs(ref["S12"])).astype(np.float32)).astype(np.float64)
    fdiff = np.abs(T.astype(np.float64) - ref["S12"].astype(np.float64))
    print("%s: S = %.3e, kernel - restatement = %.3e (%.2f S), float matrix equal: %s" % (name, dev, diff, diff / dev if dev else 0.0,
                                                                                       (T == ref["S12"]).all()))
    print("%s: iterations %s / %s, trials %s / %s (kernel / restatement), min |rho| %s" % (
        name, info["iterations"], ref["iterations"], info["trials"], ref["trials"], ["%.1e" % t["min_abs_rho"] for t in ref["trace"]]))
    assert diff <= 64 * dev, (diff, dev)
    assert (fdiff <= ulp + 64 * dev).all(), (T, ref["S12"])
    for r, tr in enumerate(ref["trace"]):
        if tr["min_abs_rho"] > 1e-6:      # at convergence the sign of rho is rounding noise, and either branch gives the same estimate
            assert (info["iterations"][r], info["trials"][r]) == (ref["iterations"][r], ref["trials"][r]), r
    assert all(info["iterations"][r] == 0 and info["trials"][r] == 0 for r in range(ref["rounds"], 2))


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernel_against_restatement(pkg, name):
    sc = S.case(name)
    res = pkg.optimize_sim3(sc["matches"], sc["prob"])
    check_against_reference(name, res)
    again = pkg.optimize_sim3(sc["matches"], sc["prob"])
    assert as_bytes(res) == as_bytes(again)                                    # determinism: identical bytes in all outputs


def test_rows_past_the_lds_stage(pkg):
    """S3O_LDS_ROWS is read from the source, so the cases cannot drift from it: the last row staged in LDS, the first read from
    memory, and more than a workgroup's worth of them - dropped and kept rows on both sides"""
    L = S.lds_rows()
    assert [len(S.case(n)["matches"]) for n in ("nL", "nL+1", "n1.3L")] == [L, L + 1, L + L * 3 // 10] and L * 3 // 10 > 256
    for name in ("nL", "nL+1", "n1.3L"):
        sc = S.case(name)
        T, dr, ni, info = pkg.optimize_sim3(sc["matches"], sc["prob"])
        ref = S.reference(name)[1]
        assert (dr[L:] == ref["dropped"][L:]).all() and (dr[:L] == ref["dropped"][:L]).all() and ni == ref["ninliers"] and info["rounds"] == 2
    d = S.reference("n1.3L")[1]["dropped"]
    assert d[L:].any() and not d[L:].all() and d[:L].any()
    # the row behind the stage decides like the same row in front of it: move it there and the result is the same set of matches
    sc = S.case("nL+1")
    perm = np.concatenate([[L], np.arange(L)])
    T2, dr2, ni2, _ = pkg.optimize_sim3(sc["matches"][perm], sc["prob"])
    assert ni2 == S.reference("nL+1")[1]["ninliers"] and (dr2 == S.reference("nL+1")[1]["dropped"][perm]).all()


def test_fixed_scale_is_bit_exact(pkg):
    sc = S.case("fix_scale65")
    T, dr, ni, info = pkg.optimize_sim3(sc["matches"], sc["prob"])
    assert info["rounds"] == 2 and ni > 40
    assert np.float64(info["s"]).tobytes() == np.float64(np.float32(sc["prob"]["s"])).tobytes()
    start = R.Sim3.from_Rts(sc["prob"]["R"], sc["prob"]["t"], sc["prob"]["s"])
    assert np.abs(info["q"] - start.q).max() > 1e-4


@pytest.mark.parametrize("name", ["drop_below10", "n9", "n0"])
def test_early_return_leaves_the_sim3_as_it_came(pkg, name):
    sc = S.case(name)
    T, dr, ni, info = pkg.optimize_sim3(sc["matches"], sc["prob"])
    start = R.Sim3.from_Rts(sc["prob"]["R"], sc["prob"]["t"], sc["prob"]["s"])
    assert ni == 0 and info["rounds"] == (0 if name == "n0" else 1)
    assert info["q"].tobytes() == start.q.tobytes() and info["t"].tobytes() == start.t.tobytes()
    assert np.float64(info["s"]).tobytes() == np.float64(start.s).tobytes() and T.tobytes() == start.matrix().tobytes()
    if name == "drop_below10":
        assert list(dr) == [1] * 6 + [0] * 8 and info["bad"] == 6 and info["iterations"][0] > 0      # the first round's drops are applied


def batch_of(names, Ks=None):
    scs = [S.case(n) for n in names]
    probs = np.array([s["prob"] for s in scs])
    if Ks is not None:
        for b, k in enumerate(Ks):
            probs["K1"][b] = np.float32(k) * probs["K1"][b]
            probs["K2"][b] = probs["K2"][b] / np.float32(k)
    m = np.concatenate([s["matches"] for s in scs])
    off = np.cumsum([0] + [len(s["matches"]) for s in scs]).astype(np.int32)
    return scs, probs, m, off


def test_batch_equals_single_calls(pkg):
    """[n9, out65, empty, nL+1, clean64] with a different K per problem, the rows starting at offsets[0] = 3"""
    names = ["n9", "out65", "n0", "nL+1", "clean64"]
    scs, probs, m, off = batch_of(names, Ks=[1.0, 1.001, 1.002, 0.999, 1.003])
    pad = np.concatenate([m[:3], m])
    Ts, dr, ni, infos = pkg.optimize_sim3_batch(pad, off + 3, probs)
    assert (dr[:3] == 0).all()                                                                   # rows before offsets[0] are not touched
    for b, s in enumerate(scs):
        one = pkg.optimize_sim3(s["matches"], probs[b])
        assert as_bytes(one) == as_bytes((Ts[b], dr[3 + off[b]:3 + off[b + 1]], int(ni[b]), infos[b])), names[b]
    assert len({Ts[b].tobytes() for b in range(5)}) == 5
    # the unscaled problems are the cases of test_kernel_against_restatement: every kind of return in one launch
    scs, probs, m, off = batch_of(names)
    Ts, dr, ni, infos = pkg.optimize_sim3_batch(m, off, probs)
    for b, n in enumerate(names):
        check_against_reference(n, (Ts[b], dr[off[b]:off[b + 1]], int(ni[b]), infos[b]))
    assert [(i["rounds"], i["bad"] > 0) for i in infos] == [(1, False), (2, True), (0, False), (2, True), (2, False)]
    Ts, dr, ni, infos = pkg.optimize_sim3_batch(m[:0], [0], probs[:0])                           # B = 0
    assert len(Ts) == 0 and len(ni) == 0 and infos == []


def regrowing_batch(pkg):
    """-> (names, scenes, problems, matches, offsets) of a batch whose rows alone exceed the staging pair's 256 KiB floor"""
    n_big = len(S.case("n1.3L")["matches"])
    K = (1 << 18) // (48 * n_big) + 1
    assert pkg.SIM3OPT_MATCH_DTYPE.itemsize == 48 and (K - 1) * 48 * n_big <= 1 << 18 < K * 48 * n_big
    names = ["out65"] + ["n1.3L"] * K + ["n9", "nL"]
    return (names,) + batch_of(names)


def test_batch_past_the_floor_from_a_fresh_thread(pkg):
    """After out65 alone reserved the pair at its floor, the batch regrows it; every problem equals its single call; the release
    returns OK and the next call gives equal bytes."""
    names, scs, probs, m, off = regrowing_batch(pkg)
    got = {}

    def worker():
        try:
            got["first"] = as_bytes(pkg.optimize_sim3(scs[0]["matches"], probs[0]))
            got["batch"] = pkg.optimize_sim3_batch(m, off, probs)
            got["again"] = as_bytes(pkg.optimize_sim3(scs[0]["matches"], probs[0]))
            got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
            got["after"] = as_bytes(pkg.optimize_sim3(scs[0]["matches"], probs[0]))
            got["rc2"] = pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001
            got["error"] = e

    th = threading.Thread(target=worker)
    th.start(); th.join()
    assert "error" not in got, got.get("error")
    one = {n: as_bytes(pkg.optimize_sim3(S.case(n)["matches"], S.case(n)["prob"])) for n in set(names)}
    Ts, dr, ni, infos = got["batch"]
    for b, n in enumerate(names):
        assert as_bytes((Ts[b], dr[off[b]:off[b + 1]], int(ni[b]), infos[b])) == one[n], (b, n)
    assert got["first"] == got["again"] == got["after"] == one["out65"] and got["rc"] == got["rc2"] == pkg.ORBX_OK


from test_scratch_fill_gpu import PAIR_BLOCKS, fill      # noqa: E402,F401   the fixture that fills every fresh scratch block


def test_results_do_not_depend_on_fresh_scratch(pkg, fill):      # noqa: F811
    """out65 and the regrowing batch with every new scratch block filled with two different words give the
    bytes of the run without a fill"""
    sc = S.case("out65")

    def run_one():
        res = pkg.optimize_sim3(sc["matches"], sc["prob"])
        return {"bytes": dict(enumerate(as_bytes(res))), "res": res}
    fill.three(run_one, PAIR_BLOCKS, lambda raw: check_against_reference("out65", raw["res"]), "Sim3 optimisation")
    names, scs, probs, m, off = regrowing_batch(pkg)

    def run_batch():
        first = pkg.optimize_sim3(scs[0]["matches"], probs[0])          # the pair at its floor, then the batch regrows it: 2 + 2 blocks
        Ts, dr, ni, infos = pkg.optimize_sim3_batch(m, off, probs)
        out = {"first %d" % k: v for k, v in enumerate(as_bytes(first))}
        for b in range(len(names)):
            out.update({"problem %02d output %d" % (b, k): v for k, v in enumerate(as_bytes((Ts[b], dr[off[b]:off[b + 1]], int(ni[b]), infos[b])))})
        return out
    fill.three(run_batch, 2 * PAIR_BLOCKS, None, "Sim3 optimisation, regrowing batch")


def test_argument_errors_do_not_touch_the_device(pkg):
    L = pkg.matcher_lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    sc = S.case("n10")
    m, pr = sc["matches"].copy(), np.array([sc["prob"]] * 2)
    So = np.full((2, 4, 4), 7, np.float32); dr = np.full(10, 9, np.uint8); ni = C.c_int(-5)
    bad = m.copy(); bad["inv_sigma2_2"][9] = -0.5
    bp = pr.copy(); bp["th2"][0] = np.inf
    f = L.orbz_optimize_sim3
    assert f(p(bad), 10, p(pr), p(So), p(dr), C.byref(ni), None, 0) == pkg.ORBX_ERR_ARG
    assert f(p(m), 10, p(bp), p(So), p(dr), C.byref(ni), None, 0) == pkg.ORBX_ERR_ARG
    assert f(None, 10, p(pr), p(So), p(dr), C.byref(ni), None, 0) == pkg.ORBX_ERR_ARG
    assert f(p(m), -1, p(pr), p(So), p(dr), C.byref(ni), None, 0) == pkg.ORBX_ERR_ARG
    assert L.orbz_optimize_sim3_batch(p(m), p(np.array([0, 6, 5], np.int32)), 2, p(pr), p(So), p(dr), p(np.zeros(2, np.int32)), None, 0) == pkg.ORBX_ERR_ARG
    # device 99 does not exist: a call that got as far as the device would say so instead
    assert f(p(bad), 10, p(pr), p(So), p(dr), C.byref(ni), None, 99) == pkg.ORBX_ERR_ARG
    assert (So == 7).all() and (dr == 9).all() and ni.value == -5
