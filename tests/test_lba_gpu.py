"""GPU: the k_lba_* kernels and their host driver (orbb_*, csrc/orbx_lba.hip) against the numpy restatement tests/lba_ref.py, at the
shapes of tests/lba_scene.py: CASES.  Erase flags, rounds, free poses and counts equal; the double estimates within 64 x S, where S
is the deviation the restatement itself shows over 16 draws of (summation order, sin / cos moved by +-2 ulp) - the kernels differ
from it by their summation order and by the device's sin / cos / sqrt; the float outputs within 1 ulp + 64 x S; iterations and
trials equal whenever that round's min |rho| > 1e-6; two runs byte-identical; the stop flag at each place the reference reads it,
and at every poll of a round that rejects four trials in a row;
Optimizer::BundleAdjustment's schedule; argument errors; a second host thread after orbx_thread_release_scratch.

Measured on one MI355X (S from the restatement alone; the difference is max |kernels - restatement| over every double estimate -
q, t of every keyframe, xyz of every point; iterations and trials are kernels / restatement per round; every case gave the same
bytes twice):
    case                         S          difference            iterations            trials
    mono                         3.197e-14  2.487e-14  0.78 S  5 4       / 5 4       5 4       / 5 4
    stereo                       7.603e-13  6.040e-13  0.79 S  5 5       / 5 5       5 5       / 5 5
    mixed                        6.590e-13  4.583e-13  0.70 S  5 4       / 5 4       5 4       / 5 4
    outliers                     2.792e-09  2.194e-09  0.79 S  5 9       / 5 9       5 10      / 5 10
    behind                       4.394e-11  1.295e-11  0.29 S  5 4       / 5 4       5 4       / 5 4
    grazing                      1.883e-13  1.457e-13  0.77 S  5 9       / 5 9       5 9       / 5 9
    dead_point                   2.487e-14  1.066e-14  0.43 S  5 4       / 5 4       5 4       / 5 4
    dead_pose                    2.085e-12  1.755e-12  0.84 S  5 10      / 5 10      5 10      / 5 10
    id0                          2.949e-13  2.771e-13  0.94 S  5 3       / 5 3       5 3       / 5 3
    no_fixed                     6.022e-12  2.249e-12  0.37 S  5 3       / 5 3       5 3       / 5 3
    nf0                          3.730e-11  1.869e-11  0.50 S  5 5       / 5 5       5 11      / 5 11
    shuffled                     2.724e-09  8.032e-11  0.03 S  5 9       / 5 9       5 10      / 5 10
    nfL                          2.011e-12  4.263e-13  0.21 S  5 6       / 5 6       5 6       / 5 6
    nfL+1                        1.734e-12  6.857e-13  0.40 S  5 6       / 5 6       5 6       / 5 6
    wide                         4.061e-11  4.059e-11  1.00 S  5 9       / 5 9       5 9       / 5 9
    many_kf                      8.864e-13  6.199e-13  0.70 S  5 3       / 5 3       5 3       / 5 3
    turned                       7.816e-14  2.309e-14  0.30 S  5 3       / 5 3       5 3       / 5 3
    far_start                    3.485e-12  1.847e-12  0.53 S  5 3       / 5 3       5 7       / 5 7
    far_outliers                 2.529e-10  1.744e-12  0.01 S  5 6       / 5 6       5 15      / 5 15
    plane_point                  2.867e-12  8.491e-13  0.30 S  5 9       / 5 9       5 9       / 5 9
    far_start stopped at poll 8  3.485e-12  1.723e-12  0.49 S  5 0       / 5 0       5 0       / 5 0
    far_start stopped at poll 9  3.485e-12  1.847e-12  0.53 S  5 1       / 5 1       5 1       / 5 1
    far_start stopped at poll 10 3.485e-12  1.847e-12  0.53 S  5 2       / 5 2       5 2       / 5 2
    far_start stopped at poll 11 3.485e-12  1.847e-12  0.53 S  5 2       / 5 2       5 3       / 5 3
    far_start stopped at poll 12 3.485e-12  1.847e-12  0.53 S  5 2       / 5 2       5 4       / 5 4
    far_start stopped at poll 13 3.485e-12  1.847e-12  0.53 S  5 2       / 5 2       5 5       / 5 5
    far_start stopped at poll 14 3.485e-12  1.847e-12  0.53 S  5 2       / 5 2       5 6       / 5 6
    far_start stopped at poll 15 3.485e-12  1.847e-12  0.53 S  5 3       / 5 3       5 7       / 5 7
    outliers stopped at 1        2.792e-09  0.000e+00  0.00 S  0 0       / 0 0       0 0       / 0 0
    outliers stopped at 2        2.792e-09  3.553e-15  0.00 S  1 0       / 1 0       1 0       / 1 0
    outliers stopped at 3        2.792e-09  4.228e-13  0.00 S  5 0       / 5 0       5 0       / 5 0
    outliers stopped at 4        2.792e-09  5.791e-13  0.00 S  5 1       / 5 1       5 1       / 5 1
    outliers stopped at 0        2.792e-09  2.194e-09  0.79 S  5 9       / 5 9       5 10      / 5 10
    initial map, robust True     1.023e-12  5.613e-13  0.55 S  12 0      / 12 0      12 0      / 12 0
    initial map, robust False    1.002e-12  4.050e-13  0.40 S  12 0      / 12 0      12 0      / 12 0
(`stopped at k`: the flag set at :655 (1), inside round 1 (2), at :664 (3), inside round 2 (4), never (0).  `stopped at poll k`: the
flag set at the k-th poll of the call; far_start's round 2 is ArrrrAA and its polls are 8 and 9 (the loop's condition before
iterations 0 and 1), 10 to 13 (after the first to fourth rejected trial of iteration 1), 14 (before iteration 2) and 15 (the
condition read once more after the loop has ended by _nBad).  The calls stopped at polls 10 to 13 return the bytes of the call stopped
at poll 9 in every estimate: a popped trial leaves nothing.)
The float outputs differ from the restatement's in their last place at most.  The rounds whose min |rho| is at or below 1e-6
(far_outliers' round 2: its last trial has |rho| = 6.3e-09) are not compared in their counts, which agreed all the same; plane_point's
round 1 (five failed solves, five NaN rho, reported as min |rho| = 0) is compared unconditionally.  far_start's rejecting iteration has
min |rho| = 4.0e-02, far_outliers' iterations rrA are decisive too.
"""
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lba_ref as R        # noqa: E402
import lba_scene as S      # noqa: E402
from test_lba_cpu import StopAt, stop_positions      # noqa: E402

pytestmark = pytest.mark.gpu
MARGIN = S.MARGIN


def as_bytes(res):
    T, X, er, info, ke, pe = res
    return (T.tobytes(), X.tobytes(), er.tobytes(), tuple(sorted((k, str(v)) for k, v in info.items())), ke.tobytes(), pe.tobytes())


def compare(name, res, ref, dev, exempt=None, counts_always=False):
    """the comparison of the module's docstring; ref: the restatement's result, dev: S.  exempt [E] bool: the edges left out of the
    depth condition (S.depth_exempt: plane_point's one edge whose depth is an exact 0.0 by construction - z > 0 on an exact zero is
    not decided by rounding).  counts_always: compare iterations and trials in every round (S.COUNTS_ALWAYS: plane_point's NaN rho is
    reported as min |rho| = 0, and a NaN is no noise about zero: both sides must reject on it)."""
    T, X, er, info, ke, pe = res
    for cl in ref["trace_class"]:      # the condition (asserted per draw in tests/test_lba_cpu.py): no edge within the margin of its threshold
        depth = cl["depth"] if exempt is None else cl["depth"][~exempt]
        assert cl["min_margin"] > MARGIN and (len(depth) == 0 or depth.min() > MARGIN), "scene %s: an edge is at its threshold - choose another seed" % name
    for k in ("rounds", "free_poses", "stopped_at", "stop_poll", "polls", "erased"):
        assert info[k] == ref["info"][k], (k, info[k], ref["info"][k])
    assert (er == ref["erase"]).all()
    got, want = np.concatenate([ke.reshape(-1), pe.reshape(-1)]), S.estimates(ref)
    diff = float(np.abs(got - want).max()) if len(got) else 0.0
    print("%s: S = %.3e, kernels - restatement = %.3e (%.2f S); iterations %s / %s, trials %s / %s (kernels / restatement), min |rho| %s" % (
        name, dev, diff, diff / dev if dev else 0.0, info["iterations"], ref["info"]["iterations"], info["trials"], ref["info"]["trials"],
        ["%.1e" % t["min_abs_rho"] for t in ref["trace"]]))
    assert diff <= 64 * dev, (diff, dev)
    for a, b in ((T, ref["Tcw"]), (X, ref["pts"])):
        ulp = np.spacing(np.maximum(np.float32(1), np.abs(b)).astype(np.float32)).astype(np.float64)
        assert (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulp + 64 * dev).all()
    for r, tr in enumerate(ref["trace"]):
        if counts_always or tr["min_abs_rho"] > 1e-6:      # at convergence the sign of rho is rounding noise, and either branch gives the same estimate
            assert (info["iterations"][r], info["trials"][r]) == (ref["info"]["iterations"][r], ref["info"]["trials"][r]), r


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernels_against_restatement(pkg, name):
    sc, ref, draws, dev = S.reference(name)
    res = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])
    compare(name, res, ref, dev, exempt=S.depth_exempt(name), counts_always=name in S.COUNTS_ALWAYS)
    again = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])
    assert as_bytes(res) == as_bytes(again)                                    # determinism: identical bytes in all outputs
    fixed = sc["kfs"]["fixed"] != 0
    assert res[0][fixed].tobytes() == sc["kfs"]["Tcw"][fixed].tobytes()        # a fixed keyframe goes out byte for byte


def test_lds_constant_is_the_sources_and_both_sides_run(pkg):
    """LBA_LDS_POSES is read from the source, so the cases cannot drift from it: the last system factorised in LDS and the first
    factorised in device memory"""
    L = S.lds_poses()
    for name, nf in (("nfL", L), ("nfL+1", L + 1)):
        sc = S.case(name)
        info = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])[3]
        assert info["free_poses"] == [nf, nf] and info["rounds"] == 2


def test_shuffled_observations_give_the_same_flags(pkg):
    """the observations of `outliers` in another order: the same erase flags edge for edge, the estimates equal up to S"""
    a, b = S.case("outliers"), S.case("shuffled")
    ra = pkg.local_bundle_adjustment(a["kfs"], a["pts"], a["obs"])
    rb = pkg.local_bundle_adjustment(b["kfs"], b["pts"], b["obs"])
    key = lambda o: np.lexsort((o["pt"], o["kf"]))      # noqa: E731
    assert (ra[2][key(a["obs"])] == rb[2][key(b["obs"])]).all() and ra[3]["erased"] == rb[3]["erased"]
    dev = max(S.reference("outliers")[3], S.reference("shuffled")[3])
    assert np.abs(ra[4] - rb[4]).max() <= 64 * dev and np.abs(ra[5] - rb[5]).max() <= 64 * dev


@pytest.mark.parametrize("where", [R.STOP_BEFORE, R.STOP_ROUND1, R.STOP_BETWEEN, R.STOP_ROUND2, 0])
def test_stop_flag_at_each_place_the_reference_reads_it(pkg, where):
    """stop at poll k, for k at :655, inside round 1, at :664 and inside round 2, and a callable that never fires: each equals the
    restatement stopped at the same poll, and the number of polls equals the restatement's"""
    sc, _, _, dev = S.reference("outliers")
    at, total = stop_positions("outliers")
    k = at[where] if where else -1
    ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"], stop=StopAt(k))
    st = StopAt(k)
    res = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], stop=st)
    assert st.calls == ref["info"]["polls"] == res[3]["polls"] and res[3]["stopped_at"] == where
    compare("outliers stopped at %d" % where, res, ref, dev)
    if where == R.STOP_BEFORE:      # nothing written
        assert res[0].tobytes() == sc["kfs"]["Tcw"].tobytes() and not res[2].any()
        assert res[1].tobytes() == np.stack([sc["pts"]["x"], sc["pts"]["y"], sc["pts"]["z"]], 1).tobytes()


def round2_polls(name):
    """-> (first, total, kinds): the number of round 2's first poll, the number of polls of an unstopped call, and per poll of
    round 2 (from `first` on) what it is: ("open", i) the poll of the loop's condition before iteration i, ("trial", i, q) the poll
    after the q-th rejected trial of iteration i (`if (more && poll(where))`), ("close",) the condition read once more after the
    loop has ended by itself.  Rebuilt from the restatement's trace, and checked against the number of polls it made."""
    sc, ref, _, _ = S.reference(name)
    calls = []
    r = R.optimize(sc["kfs"], sc["pts"], sc["obs"], stop=lambda: bool(calls.append(1)))
    t1, t2 = r["trace"]
    assert t1["trials_it"] == [1] * 5      # round 1: five iterations of one trial, so five polls and no sixth read of the condition
    first = 1 + 5 + 1 + 1                  # :655, round 1's polls, :664, then round 2's first
    kinds = []
    for i, q in enumerate(t2["trials_it"]):
        kinds.append(("open", i))
        rejected = [x < 0.0 for x in t2["rhos_it"][i]]
        kinds += [("trial", i, k + 1) for k in range(q) if rejected[k] and k + 1 < R.MAX_TRIALS]
    if t2["iterations"] < R.schedule_local()["iterations"][1]:
        kinds.append(("close",))
    assert first - 1 + len(kinds) == r["info"]["polls"] == len(calls), (first, len(kinds), r["info"]["polls"])
    return first, r["info"]["polls"], kinds


def test_stop_flag_at_every_poll_of_a_rejecting_round(pkg):
    """far_start's round 2 is ArrrrAA: its second iteration rejects four times before it accepts.  The flag set at every poll of
    that round in turn - the loop's condition and the poll between two trials alike: the call equals the restatement stopped at the
    same poll, in polls, stop_poll, stopped_at and under compare().  A stop between two rejected trials returns the estimates from
    before the iteration's first trial (every trial so far was popped): the double estimates are byte-identical to those of the call
    stopped at the poll that opens that iteration."""
    name = "far_start"
    sc, full, _, dev = S.reference(name)
    assert ["".join("A" if a else "r" for a in t["accepted"]) for t in full["trace"]] == ["AAAAA", "ArrrrAA"]
    first, total, kinds = round2_polls(name)
    assert [k[0] for k in kinds] == ["open", "open", "trial", "trial", "trial", "trial", "open", "close"]
    got = {}
    for n, kind in enumerate(kinds):
        k = first + n
        ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"], stop=StopAt(k))
        st = StopAt(k)
        res = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], stop=st)
        info = res[3]
        assert st.calls == ref["info"]["polls"] == info["polls"], (kind, st.calls, ref["info"]["polls"], info["polls"])
        assert info["stop_poll"] == ref["info"]["stop_poll"] == k and info["stopped_at"] == ref["info"]["stopped_at"] == R.STOP_ROUND2
        assert (info["iterations"], info["trials"]) == (ref["info"]["iterations"], ref["info"]["trials"]), (kind, info, ref["info"])
        compare("%s stopped at poll %d %s" % (name, k, kind), res, ref, dev)
        got[kind] = res
    for kind in kinds:
        if kind[0] == "trial":      # nothing of the iteration's rejected trials stays
            opened = got[("open", kind[1])]
            assert got[kind][4].tobytes() == opened[4].tobytes() and got[kind][5].tobytes() == opened[5].tobytes(), kind
            assert got[kind][0].tobytes() == opened[0].tobytes() and got[kind][1].tobytes() == opened[1].tobytes()
            assert got[kind][3]["trials"][1] == opened[3]["trials"][1] + kind[2] and got[kind][3]["iterations"][1] == opened[3]["iterations"][1] + 1
    assert got[("open", 0)][4].tobytes() != got[("open", 1)][4].tobytes() != got[("open", 2)][4].tobytes()      # the accepted trials do move them


def test_a_raising_stop_callable_ends_the_call(pkg):
    sc = S.case("mono")

    def boom():
        raise KeyError("stop")
    with pytest.raises(KeyError):
        pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], stop=boom)


@pytest.mark.parametrize("robust", [True, False])
def test_bundle_adjustment_on_an_initial_map(pkg, robust):
    """orbb_bundle_adjustment on a two-keyframe map, keyframe 0 fixed: GlobalBundleAdjustemnt(mpMap, 20)"""
    sc = S.initial_map()
    ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"], schedule=R.schedule_global(20, robust))
    rng = np.random.default_rng(99)
    draws = [R.optimize(sc["kfs"], sc["pts"], sc["obs"], schedule=R.schedule_global(20, robust), order=rng, perturb=rng) for _ in range(S.DRAWS)]
    dev = max(float(np.abs(S.estimates(d) - S.estimates(ref)).max()) for d in draws)
    res = pkg.bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], iterations=20, robust=robust)
    compare("initial map, robust %s" % robust, res, ref, dev)
    assert not res[2].any() and res[0][0].tobytes() == sc["kfs"]["Tcw"][0].tobytes()
    assert as_bytes(res) == as_bytes(pkg.bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], iterations=20, robust=robust))
    sched = R.schedule_global(20, robust)
    rec = pkg.lba_schedule(sched["rounds"], sched["iterations"], sched["robust"], sched["delta_mono"], sched["delta_stereo"], 0, 0)
    assert as_bytes(pkg.bundle_adjustment_scheduled(sc["kfs"], sc["pts"], sc["obs"], rec)) == as_bytes(res)


def test_empty_and_edgeless_problems(pkg):
    sc = S.case("mono")
    T, X, er, info, ke, pe = pkg.local_bundle_adjustment(sc["kfs"][:0], sc["pts"][:0], sc["obs"][:0])
    assert len(T) == 0 and len(X) == 0 and len(er) == 0 and info["iterations"] == [0, 0] and info["rounds"] == 2
    T, X, er, info, ke, pe = pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"][:0])
    ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"][:0])
    assert T.tobytes() == ref["Tcw"].tobytes() and X.tobytes() == ref["pts"].tobytes() and info == ref["info"]
    assert ke.tobytes() == ref["kf_est"].tobytes() and pe.tobytes() == ref["pt_est"].tobytes()


def test_argument_errors_do_not_touch_the_device(pkg):
    L = pkg.matcher_lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    sc = S.case("mono")
    kf, pt, ob = sc["kfs"].copy(), sc["pts"].copy(), sc["obs"].copy()
    K, P, E = len(kf), len(pt), len(ob)
    To, Po, er = np.full((K, 16), 7, np.float32), np.full((P, 3), 7, np.float32), np.full(E, 9, np.uint8)
    nostop = pkg.LBA_STOP_FN()
    f = L.orbb_local_bundle_adjustment
    bad = ob.copy(); bad[7] = bad[3]
    assert f(p(kf), K, p(pt), P, p(bad), E, nostop, None, p(To), p(Po), p(er), None, None, None, 0) == pkg.ORBX_ERR_ARG
    bad = ob.copy(); bad["kf"][1] = K
    assert f(p(kf), K, p(pt), P, p(bad), E, nostop, None, p(To), p(Po), p(er), None, None, None, 0) == pkg.ORBX_ERR_ARG
    bad = ob.copy(); bad["u"][1] = np.nan
    assert f(p(kf), K, p(pt), P, p(bad), E, nostop, None, p(To), p(Po), p(er), None, None, None, 0) == pkg.ORBX_ERR_ARG
    assert f(p(kf), K, p(pt), P, p(ob), E, nostop, None, None, p(Po), p(er), None, None, None, 0) == pkg.ORBX_ERR_ARG
    # device 99 does not exist: a call that got as far as the device would say so instead
    bad = ob.copy(); bad["inv_sigma2"][0] = -1
    assert f(p(kf), K, p(pt), P, p(bad), E, nostop, None, p(To), p(Po), p(er), None, None, None, 99) == pkg.ORBX_ERR_ARG
    assert f(p(kf), K, p(pt), P, p(ob), E, nostop, None, p(To), p(Po), p(er), None, None, None, 99) == pkg.ORBX_ERR_NO_DEVICE
    assert (To == 7).all() and (Po == 7).all() and (er == 9).all()


def test_second_host_thread_after_release(pkg):
    """scratch is per host thread: another thread gets the same bytes, releases its scratch, and gets them again"""
    sc = S.case("mixed")
    here = as_bytes(pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"]))
    got = {}

    def worker():
        try:
            got["first"] = as_bytes(pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"]))
            got["rc"] = pkg.matcher_lib().orbx_thread_release_scratch()
            got["after"] = as_bytes(pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"]))
            got["rc2"] = pkg.matcher_lib().orbx_thread_release_scratch()
        except Exception as e:      # noqa: BLE001
            got["error"] = e
    th = threading.Thread(target=worker)
    th.start(); th.join()
    assert "error" not in got, got.get("error")
    assert got["first"] == got["after"] == here and got["rc"] == got["rc2"] == pkg.ORBX_OK
    assert as_bytes(pkg.local_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])) == here
