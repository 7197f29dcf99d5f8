"""GPU: the blocked reduced-system path (k_gba_schur, k_gba_diag / rows / trail, the blocked substitutions; csrc/orbx_lba.hip) through
orbb_global_bundle_adjustment and orbb_optimize_blocked, against the numpy restatement tests/lba_ref.py under the comparison of
tests/test_lba_gpu.py (compare): the double estimates within 64 x S, S being the restatement's own spread over 16 draws of summation
order and sin / cos +-2 ulp; the floats within 1 ulp + 64 S; the counts equal where min |rho| > 1e-6; erase flags, rounds, free
poses and stop position equal.  The scenes of tests/gba_scene.py under the global schedule (a partial panel, one panel, two and a
remainder, structurally zero blocks with a loop block, a sum longer than its owner's 256 threads and a block of one contribution),
and EVERY scene of tests/lba_scene.py under the local schedule on the blocked path: dead poses, two rounds, no free pose, the failed
pivot.  Two calls give the same bytes; a fixed keyframe goes out byte for byte; fresh scratch filled with a word changes nothing (S
is cleared before every trial); the stop flag at a poll inside the round; argument errors leave the outputs alone."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gba_scene as GS     # noqa: E402
import lba_ref as R        # noqa: E402
import lba_scene as S      # noqa: E402
from test_lba_cpu import StopAt      # noqa: E402
from test_lba_gpu import as_bytes, compare      # noqa: E402
from test_scratch_fill_gpu import PAIR_BLOCKS, fill      # noqa: E402,F401   the fixture that fills every fresh scratch block

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(GS.CASES))
def test_global_bundle_adjustment_against_restatement(pkg, name):
    sc, ref, _, dev = GS.reference(name)
    res = pkg.global_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])
    compare(name, res, ref, dev)
    info = res[3]
    nb, nc, _ = GS.pattern(sc)
    nf = len(sc["kfs"]) - 1
    assert (info["blocks"], info["contributions"], info["panels"]) == ([nb, 0], [nc, 0], [-(-nf // GS.panel_poses()), 0]), info
    assert info["launches"] > 0 and not res[2].any()
    again = pkg.global_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])
    assert as_bytes(res) == as_bytes(again)                                    # determinism: identical bytes in all outputs
    assert res[0][0].tobytes() == sc["kfs"]["Tcw"][0].tobytes()                # the fixed keyframe goes out byte for byte


@pytest.mark.parametrize("name", list(S.CASES))
def test_blocked_path_on_every_local_scene(pkg, name):
    """orbb_optimize_blocked under LocalBundleAdjustment's schedule against the reference the existing tests use"""
    sc, ref, _, dev = S.reference(name)
    res = pkg.bundle_adjustment_scheduled(sc["kfs"], sc["pts"], sc["obs"], pkg.lba_schedule(), blocked=True)
    compare(name + " (blocked)", res, ref, dev, exempt=S.depth_exempt(name), counts_always=name in S.COUNTS_ALWAYS)
    assert res[3]["panels"] == [-(-nf // GS.panel_poses()) for nf in ref["info"]["free_poses"]]
    fixed = sc["kfs"]["fixed"] != 0
    assert res[0][fixed].tobytes() == sc["kfs"]["Tcw"][fixed].tobytes()


def test_panel_constant_is_the_sources(pkg):
    """GBA_PANEL_POSES is read from the source: one partial panel, exactly one, two and a remainder"""
    G = GS.panel_poses()
    for name, nf in (("one_short", G - 1), ("one_panel", G), ("two_and_rest", 2 * G + 3)):
        sc = GS.case(name)
        info = pkg.global_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])[3]
        assert info["free_poses"][0] == nf and info["panels"][0] == -(-nf // G), info


def test_blocked_and_dense_paths_agree(pkg):
    """bundle_adjustment (one workgroup factorises) and global_bundle_adjustment on the same scene: the same counts, the estimates
    within the comparison's bound of each other's reference"""
    sc, ref, _, dev = GS.reference("two_and_rest")
    a = pkg.bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], iterations=GS.ITERATIONS, robust=False)
    b = pkg.global_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])
    compare("two_and_rest (dense path)", a, ref, dev)
    assert a[3]["iterations"] == b[3]["iterations"] and a[3]["trials"] == b[3]["trials"]
    assert np.abs(a[4] - b[4]).max() <= 128 * dev and np.abs(a[5] - b[5]).max() <= 128 * dev


def test_stop_flag_at_a_poll_inside_the_round(pkg):
    sc, _, _, dev = GS.reference("window_loop")
    ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"], schedule=GS.schedule(), stop=StopAt(3))
    st = StopAt(3)
    res = pkg.global_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], stop=st)
    assert st.calls == ref["info"]["polls"] == res[3]["polls"] and res[3]["stopped_at"] == R.STOP_ROUND1 and res[3]["iterations"] == [2, 0]
    compare("window_loop stopped at poll 3", res, ref, dev)


@pytest.mark.parametrize("name", ["window_loop", "one_short"])
def test_results_do_not_depend_on_fresh_scratch(pkg, fill, name):      # noqa: F811
    """every fresh scratch block filled with two different words: the bytes of the run without a fill.  S is device-only memory that
    the pattern's blocks cover in part: a forgotten clear would leave the fill word in the structurally zero blocks"""
    sc, ref, _, dev = GS.reference(name)

    def run():
        res = pkg.global_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"])
        return {"bytes": dict(enumerate(as_bytes(res))), "res": res}
    fill.three(run, PAIR_BLOCKS, lambda raw: compare(name, raw["res"], ref, dev), "global bundle adjustment " + name)


def test_argument_errors_do_not_touch_the_device(pkg):
    L = pkg.matcher_lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    sc = GS.case("one_short")
    kf, pt, ob = sc["kfs"].copy(), sc["pts"].copy(), sc["obs"].copy()
    K, P, E = len(kf), len(pt), len(ob)
    To, Po, er = np.full((K, 16), 7, np.float32), np.full((P, 3), 7, np.float32), np.full(E, 9, np.uint8)
    nostop = pkg.LBA_STOP_FN()
    binfo = np.full(1, 5, pkg.LBA_BLOCKED_INFO_DTYPE)
    f = L.orbb_global_bundle_adjustment
    bad = ob.copy(); bad[7] = bad[3]
    assert f(p(kf), K, p(pt), P, p(bad), E, 10, 0, nostop, None, p(To), p(Po), None, None, None, p(binfo), 0) == pkg.ORBX_ERR_ARG
    bad = ob.copy(); bad["kf"][1] = K
    assert f(p(kf), K, p(pt), P, p(bad), E, 10, 0, nostop, None, p(To), p(Po), None, None, None, p(binfo), 0) == pkg.ORBX_ERR_ARG
    bad = ob.copy(); bad["u"][1] = np.nan
    assert f(p(kf), K, p(pt), P, p(bad), E, 10, 0, nostop, None, p(To), p(Po), None, None, None, p(binfo), 0) == pkg.ORBX_ERR_ARG
    assert f(p(kf), K, p(pt), P, p(ob), E, 10, 0, nostop, None, None, p(Po), None, None, None, p(binfo), 0) == pkg.ORBX_ERR_ARG
    assert f(p(kf), K, p(pt), P, p(ob), E, pkg.LBA_MAX_ITERATIONS + 1, 0, nostop, None, p(To), p(Po), None, None, None, p(binfo), 0) == pkg.ORBX_ERR_ARG
    rec = np.array([pkg.lba_schedule(rounds=3)])
    assert L.orbb_optimize_blocked(p(kf), K, p(pt), P, p(ob), E, p(rec), nostop, None, p(To), p(Po), p(er), None, None, None, p(binfo), 0) == pkg.ORBX_ERR_ARG
    # device 99 does not exist: a call that got as far as the device would say so instead
    bad = ob.copy(); bad["inv_sigma2"][0] = -1
    assert f(p(kf), K, p(pt), P, p(bad), E, 10, 0, nostop, None, p(To), p(Po), None, None, None, p(binfo), 99) == pkg.ORBX_ERR_ARG
    assert f(p(kf), K, p(pt), P, p(ob), E, 10, 0, nostop, None, p(To), p(Po), None, None, None, p(binfo), 99) == pkg.ORBX_ERR_NO_DEVICE
    assert (To == 7).all() and (Po == 7).all() and (er == 9).all() and binfo.tobytes() == np.full(1, 5, pkg.LBA_BLOCKED_INFO_DTYPE).tobytes()


def test_empty_problem(pkg):
    sc = GS.case("one_short")
    T, X, er, info, ke, pe = pkg.global_bundle_adjustment(sc["kfs"][:0], sc["pts"][:0], sc["obs"][:0])
    assert len(T) == 0 and len(X) == 0 and info["iterations"] == [0, 0] and info["blocks"] == [0, 0]
    T, X, er, info, ke, pe = pkg.global_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"][:0])
    ref = R.optimize(sc["kfs"], sc["pts"], sc["obs"][:0], schedule=GS.schedule())
    assert T.tobytes() == ref["Tcw"].tobytes() and X.tobytes() == ref["pts"].tobytes() and ke.tobytes() == ref["kf_est"].tobytes()
