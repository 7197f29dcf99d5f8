"""CPU: the loop map correction without a GPU.  (1) Known answers of the restatement tests/mapcorrect_ref.py, and every scene shows what it is
named for.  (2) Every mutation of the restatement changes the expected output on at least one scene.  (3) The kernels' text
(csrc/orbx_mapcorrect_dev.h and orbx_mapcorrect_plan.h, -DORBX_COVIS_HOST) compiled for the host, one thread per workgroup, equals the
restatement in every output byte on every scene; the same stand-alone program under AddressSanitizer / UBSan with the runtimes linked
statically.  (4) Record sizes and constants, every argument error of the two entry points, and the no-device status."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mapcorrect_ref as MR        # noqa: E402
import mapcorrect_scene as S       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGDIR = os.path.join(ROOT, "orb_slam2v2-1_amd")
F32, F64 = np.float32, np.float64


def _build(out, extra):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKGDIR, "csrc"), "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-o", out, os.path.join(ROOT, "tests", "cpp", "mapcorrect_lockstep.cc")])
    return out


@pytest.fixture(scope="module")
def lockstep(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("bin") / "mapcorrect_lockstep"), [])


def loop_blob(sc):
    t, q = sc["table"], sc["queries"]
    hd = np.array([len(t["kf"]), len(t["pts"]), len(t["obs"]), len(t["sf"]), len(q["query_kf"]), len(q["feat"]), sc["cur"]], np.int32)
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (hd, t["kf"], t["pts"], t["obs_off"], t["obs"], t["sf"], q["query_kf"], q["feat_off"], q["feat"],
                                                               np.ascontiguousarray(sc["Tiw"], F32), np.array([sc["Scw"]], MR.SIM3_DTYPE)))


def spread_blob(sc):
    off, child = S.child_lists(sc)
    hd = np.array([len(sc["kf_in_gba"]), len(sc["bad"]), len(child), len(sc["origins"])], np.int32)
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (hd, sc["Tcw"], sc["TcwGBA"], sc["kf_in_gba"], off, child, sc["origins"], sc["pos"], sc["posGBA"],
                                                               sc["pt_in_gba"], sc["ref_kf"], sc["bad"]))


def loop_bytes(want):
    return b"".join(np.ascontiguousarray(want[k]).tobytes() for k in MR.LOOP_ARRAYS)


def spread_bytes(want):
    return b"".join(np.ascontiguousarray(want[k]).tobytes() for k in MR.SPREAD_ARRAYS) + np.array([want["levels"]], np.int32).tobytes()


def run_lockstep(exe, tmp_path, mode, blob, env=None):
    (tmp_path / "in.bin").write_bytes(blob)
    subprocess.run([exe, mode, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120, env=env)
    return (tmp_path / "out.bin").read_bytes()


# ---- (1) the restatement's known answers and the scenes
def test_identity_poses_and_a_pure_scale():
    """identity poses and Scw = (identity, t, s) with s a power of two: every corrected Sim3 is Scw itself, the new poses are
    [I, t / s] exactly, and with t = 0 an owned point goes to pos / s exactly"""
    sc = S.loop_scene("scaled")
    Tiw = np.stack([np.eye(4, dtype=F32)] * 5)
    for t in ([0.0, 0.0, 0.0], [1.0, -2.0, 3.0]):
        Scw = np.zeros(1, MR.SIM3_DTYPE)[0]
        Scw["q"], Scw["t"], Scw["s"] = [0, 0, 0, 1], t, 4.0
        got = MR.correct_loop(sc["table"], sc["queries"], S.CUR, Tiw, Scw)
        for q in range(5):
            assert got["corrected"][q].tobytes() == Scw.tobytes()
            assert (got["non_corrected"]["q"][q] == [0, 0, 0, 1]).all() and (got["non_corrected"]["t"][q] == 0).all() and got["non_corrected"]["s"][q] == 1.0
            assert (got["Tiw_new"][q, :3, :3] == np.eye(3)).all() and (got["Tiw_new"][q, :3, 3] == np.array(t, F32) / F32(4)).all()
            assert (got["Ow_new"][q] == -np.array(t, F32) / F32(4)).all()
        owned = got["corrected_ref"] >= 0
        assert owned.sum() > 200
        pos = sc["table"]["pts"]["pos"]
        if not any(t):
            assert (got["pos"][owned] == pos[owned] / F32(4)).all()
        assert (got["pos"][~owned] == pos[~owned]).all()


def test_spread_with_the_poses_unchanged():
    """TcwGBA == Tcw everywhere (poses whose products are exact): no pose changes a byte, and a moved point is the two roundings of
    Xc = Rcw pos + tcw, pos' = Rwc Xc + twc, nothing else"""
    sc = S.spread_scene("exact")
    got = S.spread_expected("exact")
    assert got["Tcw_new"].tobytes() == sc["Tcw"].tobytes() and got["TcwGBA"].tobytes() == sc["TcwGBA"].tobytes()
    moved = np.nonzero(got["status"] == MR.SPREAD_MOVED)[0]
    assert len(moved) > 50
    for p in moved:
        T = sc["Tcw"][sc["ref_kf"][p]]
        R, t, x = T[:3, :3].astype(F64), T[:3, 3].astype(F64), sc["pos"][p].astype(F64)
        Xc = np.array([((R[i, 0] * x[0] + R[i, 1] * x[1]) + R[i, 2] * x[2]) + t[i] for i in range(3)]).astype(F32).astype(F64)
        Ow = np.array([((R[0, i] * t[0] + R[1, i] * t[1]) + R[2, i] * t[2]) * -1.0 for i in range(3)]).astype(F32).astype(F64)
        want = np.array([((R[0, i] * Xc[0] + R[1, i] * Xc[1]) + R[2, i] * Xc[2]) + Ow[i] for i in range(3)]).astype(F32)
        assert got["pos"][p].tobytes() == want.tobytes()
        assert np.abs(got["pos"][p] - sc["pos"][p]).max() <= 2 * np.spacing(F32(32))      # |coordinates| < 32: two roundings there at the most


def test_loop_scenes_show_what_they_are_named_for():
    sc, want = S.loop_scene("scaled"), S.loop_expected("scaled")
    sp, qk = S.SPECIAL, list(sc["queries"]["query_kf"])
    assert qk == S.QUERY_SLOTS and qk.index(S.CUR) == 3 and qk != list(range(qk[0], qk[0] + 5))
    assert len(sc["table"]["pts"]) > 256 and len(sc["queries"]["feat"]) > 256
    obs = lambda p: list(sc["table"]["obs"]["kf"][sc["table"]["obs_off"][p]:sc["table"]["obs_off"][p + 1]])      # noqa: E731
    assert want["corrected_ref"][sp["third"]] == qk[2] and obs(sp["third"]) == [0, 1, 3, 4, 8] and want["normals"]["status"][sp["third"]] == MR.NORMAL_OK
    f3 = sc["queries"]["feat"]["point"][sc["queries"]["feat_off"][1]:sc["queries"]["feat_off"][2]]
    assert (f3 == sp["twice"]).sum() == 2 and want["corrected_ref"][sp["twice"]] == 3
    assert (sc["queries"]["feat"]["point"] == -1).any()
    assert want["corrected_ref"][sp["bad"]] == -1 and want["normals"]["status"][sp["bad"]] == MR.NORMAL_UNTOUCHED and (sc["queries"]["feat"]["point"] == sp["bad"]).any()
    assert want["normals"]["status"][sp["empty"]] == MR.NORMAL_NO_OBSERVATION and want["corrected_ref"][sp["empty"]] == 4
    assert (want["pos"][sp["empty"]] != sc["table"]["pts"]["pos"][sp["empty"]]).any()
    assert want["normals"]["status"][sp["noref"]] == MR.NORMAL_NO_REFERENCE and want["normals"]["status"][sp["strayref"]] == MR.NORMAL_NO_REFERENCE
    assert want["corrected_ref"][sp["unseen"]] == -1 and (want["pos"][sp["unseen"]] == sc["table"]["pts"]["pos"][sp["unseen"]]).all()
    assert sc["Scw"]["s"] != 1.0 and S.loop_scene("unit_scale")["Scw"]["s"] == 1.0 and S.loop_scene("q1")["Scw"]["s"] != 1.0
    assert len(S.loop_scene("q1")["queries"]["query_kf"]) == 1
    # every status of an owned point occurs, and all five owners
    assert set(want["normals"]["status"]) == {0, 2, 3, 4} and set(want["corrected_ref"]) == set(qk) | {-1}


def test_spread_scene_shows_what_it_is_named_for():
    sc, want = S.spread_scene("tree"), S.spread_expected("tree")
    assert want["levels"] == 3 and len(sc["origins"]) == 2 and len(sc["bad"]) > 256
    assert list(want["kf_marked"]) == [1] * 13 + [0]
    assert set(want["status"]) == {0, 1, 2, 3}
    st = want["status"]
    assert st[12] == MR.SPREAD_UNDEFINED and st[13] == MR.SPREAD_UNTOUCHED and st[14] == MR.SPREAD_UNDEFINED and st[17] == MR.SPREAD_UNTOUCHED
    assert all(st[k] == MR.SPREAD_MOVED for k in range(12))
    for k in (3, 4, 5, 6, 7, 11):      # outside the global BA and reached: a pose of their own
        assert want["TcwGBA"][k].tobytes() != sc["TcwGBA"][k].tobytes() and want["Tcw_new"][k].tobytes() == want["TcwGBA"][k].tobytes()
    assert want["TcwGBA"][8].tobytes() == sc["TcwGBA"][8].tobytes()      # inside, under a keyframe outside: keeps its own
    assert want["Tcw_new"][12].tobytes() == sc["Tcw"][12].tobytes() and want["Tcw_new"][13].tobytes() == sc["Tcw"][13].tobytes()


# ---- (2) the mutations
@pytest.mark.parametrize("mutation", MR.MUTATIONS)
def test_every_mutation_changes_an_expected_output(mutation):
    if mutation in MR.LOOP_MUTATIONS:
        changed = [n for n in S.LOOP_SCENES if loop_bytes(S.loop_expected(n, mutation)) != loop_bytes(S.loop_expected(n))]
    else:
        changed = [n for n in S.SPREAD_SCENES if spread_bytes(S.spread_expected(n, mutation)) != spread_bytes(S.spread_expected(n))]
    assert changed, mutation


# ---- (3) the kernels' text on the host
@pytest.mark.parametrize("name", S.LOOP_SCENES)
def test_loop_kernel_text_on_the_host_equals_the_restatement(lockstep, tmp_path, name):
    got, want = run_lockstep(lockstep, tmp_path, "loop", loop_blob(S.loop_scene(name))), loop_bytes(S.loop_expected(name))
    assert len(got) == len(want)
    at = 0
    for k in MR.LOOP_ARRAYS:
        n = S.loop_expected(name)[k].nbytes
        assert got[at:at + n] == want[at:at + n], k
        at += n


@pytest.mark.parametrize("name", S.SPREAD_SCENES)
def test_spread_kernel_text_on_the_host_equals_the_restatement(lockstep, tmp_path, name):
    got, want = run_lockstep(lockstep, tmp_path, "spread", spread_blob(S.spread_scene(name))), spread_bytes(S.spread_expected(name))
    assert len(got) == len(want)
    at = 0
    for k in MR.SPREAD_ARRAYS:
        n = S.spread_expected(name)[k].nbytes
        assert got[at:at + n] == want[at:at + n], k
        at += n
    assert got[at:] == want[at:], "levels"


def test_lockstep_program_under_sanitizers(tmp_path_factory, tmp_path):
    """the stand-alone program (its own main, no Python in the process) with -fsanitize=address,undefined, the two runtimes linked
    statically: the program puts nothing into LD_PRELOAD and the environment is passed on as it is.  Any report fails the run."""
    exe = _build(str(tmp_path_factory.mktemp("bin") / "mapcorrect_lockstep_san"),
                 ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name in S.LOOP_SCENES:
        assert run_lockstep(exe, tmp_path, "loop", loop_blob(S.loop_scene(name)), env=env) == loop_bytes(S.loop_expected(name))
    for name in S.SPREAD_SCENES:
        assert run_lockstep(exe, tmp_path, "spread", spread_blob(S.spread_scene(name)), env=env) == spread_bytes(S.spread_expected(name))


# ---- (4) the C ABI
def test_record_sizes_and_constants(pkg):
    assert pkg.MAPCORRECT_SIM3_DTYPE == MR.SIM3_DTYPE and pkg.MAPCORRECT_SIM3_DTYPE.itemsize == 64
    assert C.sizeof(pkg.MapCorrectLoopOut) == 56 and C.sizeof(pkg.MapCorrectSpreadIn) == 104 and C.sizeof(pkg.MapCorrectSpreadOut) == 56
    assert pkg.MAPCORRECT_NORMAL_UNTOUCHED == MR.NORMAL_UNTOUCHED
    assert (pkg.MAPCORRECT_SPREAD_UNTOUCHED, pkg.MAPCORRECT_SPREAD_GBA, pkg.MAPCORRECT_SPREAD_MOVED, pkg.MAPCORRECT_SPREAD_UNDEFINED) == (0, 1, 2, 3)
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for name, v in (("ORBR_NORMAL_UNTOUCHED", 4), ("ORBR_SPREAD_UNTOUCHED", 0), ("ORBR_SPREAD_GBA", 1), ("ORBR_SPREAD_MOVED", 2), ("ORBR_SPREAD_UNDEFINED", 3)):
        assert re.search(r"#define %s %d\b" % (name, v), hdr), name
    declared = sorted(set(re.findall(r"\b(orbr_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == sorted(pkg.MAPCORRECT_EXPORTS)
    assert all(hasattr(pkg.lib(), s) and hasattr(pkg.lib(developer=True), s) for s in pkg.MAPCORRECT_EXPORTS)


def _loop(pkg, sc, **kw):
    a = dict(table=sc["table"], queries=sc["queries"], cur=sc["cur"], Tiw=sc["Tiw"], Scw=sc["Scw"])
    a.update(kw)
    return pkg.correct_loop_map(a["table"], a["queries"], a["cur"], a["Tiw"], a["Scw"], device=pkg.device_count() + 7)


def _mutated(d, arr, field, at, value):
    d = {k: v.copy() for k, v in d.items()}
    if field:
        d[arr][field][at] = value
    else:
        d[arr][at] = value
    return d


LOOP_ERRORS = [("obs_kf", "table", "obs", "kf", 3, 99, "observation kf out of range"), ("obs_off", "table", "obs_off", None, 2, 0, "obs_off decreases"),
               ("ref_kf", "table", "pts", "ref_kf", 9, 12, "ref_kf out of range"), ("octave", "table", "obs", "octave", 5, 8, "observation octave out of range"),
               ("feature_point", "queries", "feat", "point", 2, 300, "feature point out of range"), ("feature_point_low", "queries", "feat", "point", 2, -2, "feature point out of range"),
               ("feat_off", "queries", "feat_off", None, 2, 0, "feat_off decreases"), ("query_kf", "queries", "query_kf", None, 4, 12, "query_kf out of range"),
               ("not_ascending", "queries", "query_kf", None, 1, 1, "query_kf not strictly ascending"), ("descending", "queries", "query_kf", None, 2, 2, "query_kf not strictly ascending")]


@pytest.mark.parametrize("m", LOOP_ERRORS, ids=[m[0] for m in LOOP_ERRORS])
def test_correct_loop_index_errors_never_reach_a_device(pkg, m):
    _, which, arr, field, at, value, words = m
    sc = S.loop_scene("scaled")
    with pytest.raises(pkg.OrbxError) as e:
        _loop(pkg, sc, **{which: _mutated(sc[which], arr, field, at, value)})
    assert e.value.status == pkg.ORBX_ERR_ARG and words in str(e.value), str(e.value)


@pytest.mark.parametrize("cur,words", [(5, "cur is not among the queries"), (-1, "cur out of range"), (12, "cur out of range")])
def test_correct_loop_cur_errors(pkg, cur, words):
    with pytest.raises(pkg.OrbxError) as e:
        _loop(pkg, S.loop_scene("scaled"), cur=cur)
    assert e.value.status == pkg.ORBX_ERR_ARG and words in str(e.value), str(e.value)


def _spread(pkg, sc, **kw):
    off, child = S.child_lists(sc)
    a = dict(Tcw=sc["Tcw"], TcwGBA=sc["TcwGBA"], kf_in_gba=sc["kf_in_gba"], child_off=off, child=child, origins=sc["origins"], pos=sc["pos"], posGBA=sc["posGBA"],
             pt_in_gba=sc["pt_in_gba"], ref_kf=sc["ref_kf"], bad=sc["bad"])
    a.update(kw)
    return pkg.spread_global_ba(device=pkg.device_count() + 7, **a)


def _spread_errors():
    sc = S.spread_scene("tree")
    off, child = S.child_lists(sc)

    def ch(at, v):
        c = child.copy()
        c[at] = v
        return c

    def of(at, v):
        o = off.copy()
        o[at] = v
        return o

    ref = sc["ref_kf"].copy()
    ref[20] = 14
    out = sc["kf_in_gba"].copy()
    out[9] = 0
    return [("two_child_lists", dict(child=ch(2, 2)), "a keyframe is in two child lists"), ("own_child_list", dict(child=ch(0, 0)), "a keyframe is in its own child list"),
            ("origin_in_a_child_list", dict(origins=np.array([0, 10], np.int32)), "an origin is in a child list"),
            ("origin_outside_the_gba", dict(kf_in_gba=out), "an origin is outside the global BA"), ("origin_repeated", dict(origins=np.array([0, 9, 0], np.int32)), "an origin is repeated"),
            ("origin_range", dict(origins=np.array([0, 14], np.int32)), "origin out of range"), ("origin_negative", dict(origins=np.array([-1], np.int32)), "origin out of range"),
            ("child_range", dict(child=ch(3, 14)), "child slot out of range"), ("child_negative", dict(child=ch(3, -1)), "child slot out of range"),
            ("child_off_start", dict(child_off=of(0, 1)), "child_off does not start at 0"), ("child_off_decreases", dict(child_off=of(4, 1)), "child_off decreases"),
            ("ref_kf", dict(ref_kf=ref), "ref_kf out of range")]


@pytest.mark.parametrize("m", _spread_errors(), ids=[m[0] for m in _spread_errors()])
def test_spread_argument_errors_never_reach_a_device(pkg, m):
    with pytest.raises(pkg.OrbxError) as e:
        _spread(pkg, S.spread_scene("tree"), **m[1])
    assert e.value.status == pkg.ORBX_ERR_ARG and m[2] in str(e.value), str(e.value)


def test_null_pointers(pkg):
    L = pkg.lib()
    assert L.orbr_correct_loop(None, None, 0, None, None, None, 0) == pkg.ORBX_ERR_ARG
    assert L.orbr_spread_global_ba(None, None, 0) == pkg.ORBX_ERR_ARG
    si, so = pkg.MapCorrectSpreadIn(), pkg.MapCorrectSpreadOut()
    assert L.orbr_spread_global_ba(C.addressof(si), C.addressof(so), 0) == pkg.ORBX_ERR_ARG      # no child_off


def test_no_device_status(pkg):
    """well-formed calls where no usable GPU is: ORBX_ERR_NO_DEVICE, after the checks; there is no CPU path"""
    with pytest.raises(pkg.OrbxError) as e:
        _loop(pkg, S.loop_scene("scaled"))
    assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
    with pytest.raises(pkg.OrbxError) as e:
        _spread(pkg, S.spread_scene("tree"))
    assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
