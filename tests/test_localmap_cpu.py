"""CPU: the local map without a GPU.  (1) Every scene of tests/localmap_scene.py shows what it is named for, on the restatement's own
result.  (2) The kernels' text (csrc/orbx_localmap_dev.h, -DORBX_COVIS_HOST) compiled for the host, one lane per wave, equals the literal
restatement tests/localmap_ref.py in every output byte on every scene; the program runs each frame twice on one state and checks that
the cleaning pass left it idle.  (3) The same stand-alone program under AddressSanitizer / UBSan with the runtimes linked statically, on
three scenes.  (4) Record sizes and constants, every index-range error of set_map and update, and the no-device status."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import localmap_ref as LR        # noqa: E402
import localmap_scene as S       # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGDIR = os.path.join(ROOT, "orb_slam2v2-1_amd")
CASES = [(n, 0) for n in S.SCENES] + [("random", s) for s in S.RANDOM_SEEDS_CPU]


def _build(out, extra):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKGDIR, "csrc"), "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-o", out, os.path.join(ROOT, "tests", "cpp", "localmap_lockstep.cc")])
    return out


@pytest.fixture(scope="module")
def lockstep(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("bin") / "localmap_lockstep"), [])


def graph_of(pkg_or_none, sc):
    co = np.zeros(len(sc["cov"]) + 1, np.int32)
    co[1:] = np.cumsum([len(c) for c in sc["cov"]])
    ho = np.zeros(len(sc["children"]) + 1, np.int32)
    ho[1:] = np.cumsum([len(c) for c in sc["children"]])
    flat = lambda ls: np.array([v for c in ls for v in c], np.int32).reshape(-1)      # noqa: E731
    return {"parent": sc["parent"], "cov_off": co, "cov": flat(sc["cov"]), "child_off": ho, "child": flat([sorted(c) for c in sc["children"]])}


def scene_blob(sc):
    t, q, g = sc["table"], sc["features"], graph_of(None, sc)
    hd = np.array([len(t["kf"]), len(t["pts"]), len(t["obs"]), len(t["sf"]), len(q["feat"]), len(g["cov"]), len(g["child"]), len(sc["frame_points"]),
                   len(sc["prev_kf"]), sc["max_keyframes"], sc["nbest"]], np.int32)
    return b"".join(a.tobytes() for a in (hd, t["kf"], t["pts"], t["obs_off"], t["obs"], t["sf"], q["feat_off"], q["feat"], g["parent"], g["cov_off"], g["cov"],
                                          g["child_off"], g["child"], sc["views"], sc["desc"], sc["frame_points"], sc["prev_kf"]))


def expected_blob(want):
    i = want["info"]
    h7 = np.array([i["empty_vote"], i["n_voted"], i["ref_kf"], i["ref_votes"], i["extension_end"], len(want["local_kf"]), len(want["local_pts"])], np.int32)
    return h7.tobytes() + b"".join(np.ascontiguousarray(want[k]).tobytes() for k in LR.ARRAYS)


def run_lockstep(exe, tmp_path, sc, env=None):
    (tmp_path / "in.bin").write_bytes(scene_blob(sc))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120, env=env)
    return (tmp_path / "out.bin").read_bytes()


@pytest.mark.parametrize("name", list(S.SCENES))
def test_scene_shows_what_it_is_named_for(name):
    S.assert_conditions(name)


@pytest.mark.parametrize("name,seed", CASES, ids=["%s%s" % (n, "_%d" % s if s else "") for n, s in CASES])
def test_kernel_text_on_the_host_equals_the_restatement(lockstep, tmp_path, name, seed):
    assert run_lockstep(lockstep, tmp_path, S.scene(name, seed)) == expected_blob(S.expected(name, seed))


def test_lockstep_program_under_sanitizers(tmp_path_factory, tmp_path):
    """the stand-alone program (its own main, no Python in the process) with -fsanitize=address,undefined, the two runtimes linked
    statically: the program puts nothing into LD_PRELOAD and the environment is passed on as it is.  Any report fails the run."""
    exe = _build(str(tmp_path_factory.mktemp("bin") / "localmap_lockstep_san"),
                 ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name in ("length_80_runs", "feature_counts_0_1_63_64_65_1025", "random"):
        assert run_lockstep(exe, tmp_path, S.scene(name), env=env) == expected_blob(S.expected(name))


# ---- (4) the C ABI
def test_record_sizes_and_constants(pkg):
    assert pkg.LOCALMAP_VIEW_DTYPE == LR.VIEW_DTYPE and pkg.LOCALMAP_VIEW_DTYPE.itemsize == 24
    assert pkg.LOCALMAP_INFO_DTYPE == LR.INFO_DTYPE and pkg.LOCALMAP_INFO_DTYPE.itemsize == 32
    assert pkg.WORLDPOINT_DTYPE == LR.WORLDPOINT_DTYPE and pkg.WORLDPOINT_DTYPE.itemsize == 40
    assert C.sizeof(pkg.LocalMapMap) == 72 and C.sizeof(pkg.LocalMapResult) == 96
    assert (pkg.LOCALMAP_END_RAN_OUT, pkg.LOCALMAP_END_LENGTH, pkg.LOCALMAP_END_PARENT) == (LR.END_RAN_OUT, LR.END_LENGTH, LR.END_PARENT)
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for name, v in (("ORBT_END_RAN_OUT", 0), ("ORBT_END_LENGTH", 1), ("ORBT_END_PARENT", 2)):
        assert "#define %s %d " % (name, v) in hdr
    import re
    declared = sorted(set(re.findall(r"\b(orbt_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))))
    assert declared == sorted(pkg.LOCALMAP_EXPORTS)
    assert all(hasattr(pkg.lib(), s) and hasattr(pkg.lib(developer=True), s) for s in pkg.LOCALMAP_EXPORTS)
    assert S.LDS_KEYFRAMES == pkg.COVIS_LDS_KEYFRAMES


def test_graph_helper(pkg):
    sc = S.scene("random")
    g, w = pkg.localmap_graph(sc["parent"], sc["cov"], [set(c) for c in sc["children"]]), graph_of(None, sc)
    for k in w:
        assert g[k].dtype == np.int32 and g[k].tobytes() == w[k].tobytes(), k
    with pytest.raises(ValueError):
        pkg.localmap_graph(sc["parent"], sc["cov"][:-1], sc["children"])


def _set(pkg, lm, sc, table=None, features=None, graph=None, views=None, desc=None):
    lm.set_map(table or sc["table"], features or sc["features"], graph or graph_of(None, sc), sc["views"] if views is None else views,
               sc["desc"] if desc is None else desc)


def _set_map_mutations():
    """(what, which of table / features / graph, field, index, value, the message's words)"""
    return [("obs_kf", "table", "obs", "kf", 3, 99, "observation kf out of range"), ("obs_off", "table", "obs_off", None, 2, 0, "obs_off decreases"),
            ("feature_point", "features", "feat", "point", 2, 3000, "feature point out of range"), ("feature_point_low", "features", "feat", "point", 2, -2, "feature point out of range"),
            ("feat_off", "features", "feat_off", None, 2, 0, "feat_off decreases"), ("query_kf", "features", "query_kf", None, 4, 5, "query_kf[q] is not q"),
            ("parent", "graph", "parent", None, 3, 60, "parent out of range"), ("parent_low", "graph", "parent", None, 3, -2, "parent out of range"),
            ("cov", "graph", "cov", None, 5, 60, "cov slot out of range"), ("cov_neg", "graph", "cov", None, 5, -1, "cov slot out of range"),
            ("cov_off_start", "graph", "cov_off", None, 0, 1, "cov_off does not start at 0"), ("cov_off_decreases", "graph", "cov_off", None, 7, 0, "cov_off decreases"),
            ("child", "graph", "child", None, 2, 60, "child slot out of range"), ("child_off_start", "graph", "child_off", None, 0, 2, "child_off does not start at 0"),
            ("child_off_decreases", "graph", "child_off", None, 9, 0, "child_off decreases")]


@pytest.mark.parametrize("m", _set_map_mutations(), ids=[m[0] for m in _set_map_mutations()])
def test_set_map_index_range_errors_never_reach_a_device(pkg, m):
    _, which, arr, field, at, value, words = m
    sc = S.scene("random")
    parts = {"table": {k: v.copy() for k, v in sc["table"].items()}, "features": {k: v.copy() for k, v in sc["features"].items()},
             "graph": {k: v.copy() for k, v in graph_of(None, sc).items()}}
    if field:
        parts[which][arr][field][at] = value
    else:
        parts[which][arr][at] = value
    with pkg.LocalMap() as lm:
        with pytest.raises(pkg.OrbxError) as e:
            _set(pkg, lm, sc, **parts)
        assert e.value.status == pkg.ORBX_ERR_ARG and words in str(e.value), str(e.value)


def test_set_map_shape_errors(pkg):
    sc = S.scene("plain")
    with pkg.LocalMap() as lm:
        q = sc["features"]
        fewer = {"query_kf": q["query_kf"][:-1], "feat_off": q["feat_off"][:-1], "feat": q["feat"]}
        with pytest.raises(pkg.OrbxError) as e:
            _set(pkg, lm, sc, features=fewer)
        assert e.value.status == pkg.ORBX_ERR_ARG and "Q == K" in str(e.value)
        L = pkg.lib()
        assert L.orbt_localmap_set_map(lm._h, None) == pkg.ORBX_ERR_ARG and L.orbt_localmap_set_map(None, None) == pkg.ORBX_ERR_ARG
        assert L.orbt_localmap_create(0, None) == pkg.ORBX_ERR_ARG
        # before any map: update has nothing to check its indices against
        with pytest.raises(pkg.OrbxError) as e:
            lm.update([0])
        assert e.value.status == pkg.ORBX_ERR_ARG and "no map" in str(e.value)
        # more keyframes than the marks' LDS bit set holds
        K = pkg.COVIS_MAX_CULL_KEYFRAMES + 1
        big = pkg.covis_table(np.zeros(K, pkg.COVIS_KEYFRAME_DTYPE), sc["table"]["pts"], np.zeros((0, 5)), sc["table"]["sf"])
        feats = {"query_kf": np.arange(K, dtype=np.int32), "feat_off": np.zeros(K + 1, np.int32), "feat": np.zeros(0, pkg.COVIS_FEATURE_DTYPE)}
        g = {"parent": np.full(K, -1, np.int32), "cov_off": np.zeros(K + 1, np.int32), "cov": np.zeros(0, np.int32), "child_off": np.zeros(K + 1, np.int32),
             "child": np.zeros(0, np.int32)}
        with pytest.raises(pkg.OrbxError) as e:
            lm.set_map(big, feats, g, sc["views"], sc["desc"])
        assert e.value.status == pkg.ORBX_ERR_UNSUPPORTED and "keyframes, at most" in str(e.value)


@pytest.mark.parametrize("what,kw,words", [
    ("frame_point", dict(frame_points=[0, 3000]), "frame point out of range"), ("frame_point_low", dict(frame_points=[-2]), "frame point out of range"),
    ("prev_kf", dict(frame_points=[0], prev_kf=[60]), "prev_kf out of range"), ("prev_kf_neg", dict(frame_points=[0], prev_kf=[2, -1]), "prev_kf out of range"),
    ("prev_kf_repeated", dict(frame_points=[0], prev_kf=[2, 5, 2]), "prev_kf repeated"), ("max_keyframes", dict(frame_points=[0], max_keyframes=-1), "bad arguments"),
    ("nbest", dict(frame_points=[0], nbest=-1), "bad arguments")])
def test_update_index_range_errors_never_reach_a_device(pkg, what, kw, words):
    """update checks its indices against the K and P of the last map whose host checks passed, whether or not that map reached a device"""
    sc = S.scene("random")
    with pkg.LocalMap(device=0 if pkg.device_count() > 0 else 3) as lm:
        try:
            _set(pkg, lm, sc)
        except pkg.OrbxError as e:
            assert pkg.device_count() == 0 and e.status == pkg.ORBX_ERR_NO_DEVICE
        assert (lm.K, lm.P) == (60, 3000)
        with pytest.raises(pkg.OrbxError) as e:
            lm.update(**kw)
        assert e.value.status == pkg.ORBX_ERR_ARG and words in str(e.value), str(e.value)


def test_no_device_status(pkg):
    """a well-formed map where no usable GPU is: ORBX_ERR_NO_DEVICE from set_map, and from a well-formed update after it; there is no
    CPU path"""
    sc = S.scene("plain")
    with pkg.LocalMap(device=pkg.device_count() + 7) as lm:
        with pytest.raises(pkg.OrbxError) as e:
            _set(pkg, lm, sc)
        assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
        with pytest.raises(pkg.OrbxError) as e:
            lm.update(sc["frame_points"])
        assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
