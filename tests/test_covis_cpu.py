"""CPU: covisibility without a GPU.  (1) Every scene of tests/covis_scene.py shows what it is named for, on the restatement's own
results.  (2) The kernels' text (csrc/orbx_covis_dev.h, -DORBX_COVIS_HOST) compiled for the host, one lane per wave, equals the literal
restatement tests/covis_ref.py in every output byte on every case but the one whose list is longer than the in-LDS sort's limit (the
radix path is HIP code with no check on the CPU; tests/test_covis_gpu.py runs it).  (3) The same stand-alone program under
AddressSanitizer / UBSan with the runtimes linked statically, once.
(4) Record sizes, the argument errors of the entry points - each index-range error among them - and the no-device status.  (5) The
normals' restatement equals host/frame_shim.h's MapPoint::UpdateNormalAndDepth, compiled, on the same scenes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import covis_ref as R        # noqa: E402
import covis_scene as S      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKGDIR = os.path.join(ROOT, "orb_slam2v2-1_amd")
EMPTY_Q = R.build_queries([], [])


def _build(out, src, extra):
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function"] + extra + [
        "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(PKGDIR, "csrc"), "-I" + os.path.join(PKGDIR, "host"), "-I" + os.path.join(ROOT, "tests", "cpp"),
        "-o", out, os.path.join(ROOT, "tests", "cpp", src)])
    return out


@pytest.fixture(scope="module")
def lockstep(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("bin") / "covis_lockstep"), "covis_lockstep.cc", [])


@pytest.fixture(scope="module")
def shim_check(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("bin") / "covis_shim_check"), "covis_shim_check.cc", [])


def table_blob(t):
    return t["kf"].tobytes() + t["pts"].tobytes() + t["obs_off"].tobytes() + t["obs"].tobytes() + t["sf"].tobytes()


def queries_blob(q):
    return q["query_kf"].tobytes() + q["feat_off"].tobytes() + q["feat"].tobytes()


def run_lockstep(exe, tmp_path, table, conn=None, cull=None, env=None):
    cq, kq = (conn or {}).get("queries", EMPTY_Q), (cull or {}).get("queries", EMPTY_Q)
    K, P, Qc, Qk = len(table["kf"]), len(table["pts"]), len(cq["query_kf"]), len(kq["query_kf"])
    cap = (conn or {}).get("cap", 0)
    hd = np.array([K, P, len(table["obs"]), len(table["sf"]), Qc, len(cq["feat"]), Qk, len(kq["feat"]), (conn or {}).get("th", 15), cap,
                   (cull or {}).get("monocular", 0), (cull or {}).get("th_obs", 3)], np.int32)
    (tmp_path / "in.bin").write_bytes(hd.tobytes() + table_blob(table) + queries_blob(cq) + queries_blob(kq))
    subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120, env=env)
    o = (tmp_path / "out.bin").read_bytes()
    sizes = [4 * Qc * cap, 4 * Qc * cap, 4 * Qc, 4 * Qc * K, 4 * Qk, 4 * Qk, 4 * Qk, P, 24 * P]
    assert len(o) == sum(sizes)
    parts, at = [], 0
    for n in sizes:
        parts.append(o[at:at + n])
        at += n
    i32 = lambda b: np.frombuffer(b, np.int32)     # noqa: E731
    return {"connections": (i32(parts[0]).reshape(Qc, cap), i32(parts[1]).reshape(Qc, cap), i32(parts[2]), i32(parts[3]).reshape(Qc, K)),
            "culling": (i32(parts[4]), i32(parts[5]), i32(parts[6]), np.frombuffer(parts[7], np.uint8)), "normals": np.frombuffer(parts[8], R.NORMAL_DTYPE)}


def assert_same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.tobytes() == np.ascontiguousarray(w).tobytes()


@pytest.mark.parametrize("kind,name", [("connections", n) for n in S.CONNECTION_CASES] + [("culling", n) for n in S.CULLING_CASES] +
                         [("normals", n) for n in S.NORMAL_CASES])
def test_scene_shows_what_it_is_named_for(kind, name):
    S.assert_conditions(kind, name)


# Every case but long_order: a list longer than ORBC_SORT_LDS takes cov_sort_radix, which is built on the 256-lane radix core of
# csrc/orbx_cloud_dev.h and lives in orbx_covis.hip, not in the host-compilable header.  So that wrapper - its loops over the tiles, the
# histogram columns, the back-to-front emit - has NO check on the CPU; tests/test_covis_gpu.py and tests/test_covis_scratch_fill_gpu.py
# run long_order on the GPU.
@pytest.mark.parametrize("name", [n for n in S.CONNECTION_CASES if n != "long_order"])
def test_connections_kernel_text_on_the_host_equals_the_restatement(lockstep, tmp_path, name):
    sc = S.CONNECTION_CASES[name]()
    assert_same(run_lockstep(lockstep, tmp_path, sc["table"], conn=sc)["connections"], S.expected_connections(sc))


@pytest.mark.parametrize("name", list(S.CULLING_CASES))
def test_culling_kernel_text_on_the_host_equals_the_restatement(lockstep, tmp_path, name):
    sc = S.CULLING_CASES[name]()
    assert_same(run_lockstep(lockstep, tmp_path, sc["table"], cull=sc)["culling"], S.expected_culling(sc))


@pytest.mark.parametrize("name", list(S.NORMAL_CASES))
def test_normals_kernel_text_on_the_host_equals_the_restatement(lockstep, tmp_path, name):
    sc = S.NORMAL_CASES[name]()
    assert run_lockstep(lockstep, tmp_path, sc["table"])["normals"].tobytes() == R.update_normal_and_depth(sc["table"]).tobytes()


def test_culling_scenes_feed_the_normals_and_connections_too(lockstep, tmp_path):
    """one table through all three bodies in one run: the random culling scene's table is the largest mixed one"""
    sc = S.CULLING_CASES["random"]()
    conn = {"queries": sc["queries"], "th": 2, "cap": 7}
    got = run_lockstep(lockstep, tmp_path, sc["table"], conn=conn, cull=sc)
    assert_same(got["connections"], S.expected_connections({"table": sc["table"], **conn}))
    assert_same(got["culling"], S.expected_culling(sc))
    assert got["normals"].tobytes() == R.update_normal_and_depth(sc["table"]).tobytes()


def test_lockstep_program_under_sanitizers(tmp_path_factory, tmp_path):
    """the stand-alone program (its own main, no Python in the process) with -fsanitize=address,undefined, the two runtimes linked
    statically: the program puts nothing into LD_PRELOAD and the environment is passed on as it is.  Any report fails the run
    (halt_on_error, -fno-sanitize-recover)."""
    exe = _build(str(tmp_path_factory.mktemp("bin") / "covis_lockstep_san"), "covis_lockstep.cc",
                 ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"])
    env = dict(os.environ, ASAN_OPTIONS="halt_on_error=1:detect_leaks=0", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    for name in ("ties", "long_lists", "K65", "Q40"):
        sc = S.CONNECTION_CASES[name]()
        assert_same(run_lockstep(exe, tmp_path, sc["table"], conn=sc, env=env)["connections"], S.expected_connections(sc))
    for name in ("point_dies", "random_long_lists"):
        sc = S.CULLING_CASES[name]()
        assert_same(run_lockstep(exe, tmp_path, sc["table"], cull=sc, env=env)["culling"], S.expected_culling(sc))
    sc = S.NORMAL_CASES["lists"]()
    assert run_lockstep(exe, tmp_path, sc["table"], env=env)["normals"].tobytes() == R.update_normal_and_depth(sc["table"]).tobytes()


@pytest.mark.parametrize("name", list(S.NORMAL_CASES))
def test_normals_restatement_equals_the_shim(shim_check, tmp_path, name):
    """host/frame_shim.h's MapPoint::UpdateNormalAndDepth on objects built from the table: the members it writes, and nothing on a
    point it leaves alone (those keep the zeros they were made with, which is what a nonzero status returns)"""
    t = S.NORMAL_CASES[name]()["table"]
    hd = np.array([len(t["kf"]), len(t["pts"]), len(t["obs"]), len(t["sf"])], np.int32)
    (tmp_path / "in.bin").write_bytes(hd.tobytes() + table_blob(t))
    subprocess.run([shim_check, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=120)
    got = np.frombuffer((tmp_path / "out.bin").read_bytes(), np.float32).reshape(-1, 5)
    ref = R.update_normal_and_depth(t)
    want = np.concatenate([ref["normal"], ref["max_distance"][:, None], ref["min_distance"][:, None]], axis=1)
    assert got.tobytes() == want.tobytes()


# ---- (4) the C ABI
def test_record_sizes_and_constants(pkg):
    for a, b, n in ((pkg.COVIS_KEYFRAME_DTYPE, R.KEYFRAME_DTYPE, 24), (pkg.COVIS_POINT_DTYPE, R.POINT_DTYPE, 20), (pkg.COVIS_OBSERVATION_DTYPE, R.OBSERVATION_DTYPE, 12),
                    (pkg.COVIS_FEATURE_DTYPE, R.FEATURE_DTYPE, 12), (pkg.COVIS_NORMAL_DTYPE, R.NORMAL_DTYPE, 24)):
        assert a == b and a.itemsize == n
    assert pkg.COVIS_LDS_KEYFRAMES == S.LDS_KEYFRAMES and pkg.COVIS_SORT_LDS == S.SORT_LDS
    hdr = open(os.path.join(ROOT, "include", "orbx.h")).read()
    for name, v in (("ORBC_LDS_KEYFRAMES", pkg.COVIS_LDS_KEYFRAMES), ("ORBC_SORT_LDS", pkg.COVIS_SORT_LDS), ("ORBC_MAX_CULL_KEYFRAMES", pkg.COVIS_MAX_CULL_KEYFRAMES)):
        assert "#define %s %d " % (name, v) in hdr
    assert C.sizeof(pkg.CovisTable) == 64 and C.sizeof(pkg.CovisQueries) == 32 and C.sizeof(pkg.CovisConnections) == 40 and C.sizeof(pkg.CovisCulling) == 40
    L = pkg.lib()
    assert all(hasattr(L, s) for s in pkg.COVIS_EXPORTS)


def test_table_helper_equals_the_restatements(pkg):
    sc = S.CULLING_CASES["random"]()
    t = sc["table"]
    off, obs = t["obs_off"], t["obs"]
    rows = [(p, obs["kf"][o], obs["idx"][o], obs["octave"][o], obs["stereo"][o]) for p in range(len(t["pts"])) for o in range(off[p], off[p + 1])]
    rows = [rows[i] for i in np.random.default_rng(0).permutation(len(rows))]
    got = pkg.covis_table(t["kf"], t["pts"], rows, t["sf"])
    for k in ("kf", "pts", "obs_off", "obs", "sf"):
        assert got[k].dtype == t[k].dtype and got[k].tobytes() == t[k].tobytes(), k
    with pytest.raises(ValueError):
        pkg.covis_table(t["kf"], t["pts"], rows + [rows[0]], t["sf"])
    q = sc["queries"]
    gq = pkg.covis_queries(q["query_kf"], [q["feat"][q["feat_off"][i]:q["feat_off"][i + 1]] for i in range(len(q["query_kf"]))])
    for k in ("query_kf", "feat_off", "feat"):
        assert gq[k].tobytes() == q[k].tobytes(), k
    pkg.covis_check(t, q, culling=True)


def test_precondition_check(pkg):
    sc = S.CULLING_CASES["chain"]()
    q = {k: v.copy() for k, v in sc["queries"].items()}
    pkg.covis_check(sc["table"], q, culling=True)
    q["feat"]["point"][0] = 5            # feature 0 of A now names point 5, whose observation by A is feature 5
    with pytest.raises(ValueError, match="does not name it"):
        pkg.covis_check(sc["table"], q, culling=True)
    t = {k: v.copy() for k, v in sc["table"].items()}
    t["obs"]["kf"][0] = 0                # point 0 is no longer observed by A (slot 1), but A's feature 0 names it
    with pytest.raises(ValueError, match="no observation by that keyframe"):
        pkg.covis_check(t, sc["queries"])


def _mutations():
    """(what, which of table / queries, field, index, value, the message's words)"""
    return [("kf", "obs", "kf", 3, 99, "observation kf out of range"), ("kf_neg", "obs", "kf", 3, -1, "observation kf out of range"),
            ("not_ascending", "obs", "kf", 1, 1, "not strictly ascending"), ("idx", "obs", "idx", 2, -4, "observation idx negative"),
            ("obs_octave", "obs", "octave", 2, 8, "observation octave out of range"), ("ref_kf", "pts", "ref_kf", 1, 8, "ref_kf out of range"),
            ("ref_kf_low", "pts", "ref_kf", 1, -2, "ref_kf out of range"), ("obs_off_start", "obs_off", None, 0, 1, "obs_off does not start at 0"),
            ("obs_off_decreases", "obs_off", None, 2, 3, "obs_off decreases"), ("query_kf", "query_kf", None, 1, 8, "query_kf out of range"),
            ("query_kf_neg", "query_kf", None, 0, -1, "query_kf out of range"), ("point", "feat", "point", 2, 10, "feature point out of range"),
            ("point_low", "feat", "point", 2, -2, "feature point out of range"), ("feat_octave", "feat", "octave", 0, 8, "feature octave out of range"),
            ("feat_octave_neg", "feat", "octave", 0, -1, "feature octave out of range"), ("feat_off_start", "feat_off", None, 0, 2, "feat_off does not start at 0"),
            ("feat_off_decreases", "feat_off", None, 2, 5, "feat_off decreases")]


@pytest.mark.parametrize("m", _mutations(), ids=[m[0] for m in _mutations()])
def test_index_range_errors_never_reach_a_kernel(pkg, m):
    """every check runs on the host before a device is touched: ORBX_ERR_ARG and a message on a machine without a GPU too"""
    _, arr, field, at, value, words = m
    sc = S.CULLING_CASES["chain"]()
    t = {k: v.copy() for k, v in sc["table"].items()}
    q = {k: v.copy() for k, v in sc["queries"].items()}
    tgt = t if arr in t else q
    if field:
        tgt[arr][field][at] = value
    else:
        tgt[arr][at] = value
    for call in (lambda: pkg.update_connections(t, q, check=False), lambda: pkg.keyframe_culling(t, q, 1, check=False)):
        with pytest.raises(pkg.OrbxError) as e:
            call()
        assert e.value.status == pkg.ORBX_ERR_ARG and words in str(e.value), str(e.value)
    if arr in t:
        with pytest.raises(pkg.OrbxError) as e:
            pkg.update_normal_and_depth(t)
        assert e.value.status == pkg.ORBX_ERR_ARG and words in str(e.value)


def test_argument_errors(pkg):
    sc = S.CULLING_CASES["chain"]()
    t, q = sc["table"], sc["queries"]
    for kw, words in ((dict(th=0), "th below 1"), (dict(cap=-1), "cap negative")):
        with pytest.raises(pkg.OrbxError) as e:
            pkg.update_connections(t, q, check=False, **kw)
        assert e.value.status == pkg.ORBX_ERR_ARG and words in str(e.value)
    twice = R.build_queries([1, 1], [q["feat"][:10], q["feat"][:10]])
    with pytest.raises(pkg.OrbxError) as e:
        pkg.keyframe_culling(t, twice, 1, check=False)
    assert e.value.status == pkg.ORBX_ERR_ARG and "query keyframe repeated" in str(e.value)
    pkg.covis_check(t, twice)            # connections accept a repeated query
    L = pkg.lib()
    ct = pkg._covis_c_table(t)
    cq = pkg._covis_c_queries(q)
    n = np.zeros(2, np.int32)
    assert L.orbc_update_connections(None, C.addressof(cq), 15, 0, None, None, n.ctypes.data, None, 0) == pkg.ORBX_ERR_ARG
    assert L.orbc_update_connections(C.addressof(ct), None, 15, 0, None, None, n.ctypes.data, None, 0) == pkg.ORBX_ERR_ARG
    assert L.orbc_update_connections(C.addressof(ct), C.addressof(cq), 15, 0, None, None, None, None, 0) == pkg.ORBX_ERR_ARG
    assert L.orbc_update_connections(C.addressof(ct), C.addressof(cq), 15, 4, None, None, n.ctypes.data, None, 0) == pkg.ORBX_ERR_ARG
    assert L.orbc_keyframe_culling(C.addressof(ct), None, 1, 3, n.ctypes.data, n.ctypes.data, n.ctypes.data, None, 0) == pkg.ORBX_ERR_ARG
    assert L.orbc_keyframe_culling(C.addressof(ct), C.addressof(cq), 1, 3, None, n.ctypes.data, n.ctypes.data, None, 0) == pkg.ORBX_ERR_ARG
    assert L.orbc_update_normal_and_depth(C.addressof(ct), None, 0) == pkg.ORBX_ERR_ARG
    bad = pkg._covis_c_table(t)
    bad.nlevels = 0
    assert L.orbc_update_normal_and_depth(C.addressof(bad), n.ctypes.data, 0) == pkg.ORBX_ERR_ARG
    # more keyframes than k_cull's LDS bitset holds: refused before a device is touched; the other two entry points have no such limit
    big = pkg.covis_table(np.zeros(pkg.COVIS_MAX_CULL_KEYFRAMES + 1, pkg.COVIS_KEYFRAME_DTYPE), t["pts"], np.zeros((0, 5)), t["sf"])
    with pytest.raises(pkg.OrbxError) as e:
        pkg.keyframe_culling(big, R.build_queries([3], [np.zeros(0, R.FEATURE_DTYPE)]), 1, check=False)
    assert e.value.status == pkg.ORBX_ERR_UNSUPPORTED and "keyframes in a culling call" in str(e.value)
    # nothing to do: no device is touched
    empty = pkg.covis_table(np.zeros(0, pkg.COVIS_KEYFRAME_DTYPE), np.zeros(0, pkg.COVIS_POINT_DTYPE), np.zeros((0, 5)), t["sf"])
    assert len(pkg.update_normal_and_depth(empty)) == 0


def test_no_device_status(pkg):
    """a well-formed call where no usable GPU is: ORBX_ERR_NO_DEVICE, there is no CPU path"""
    if pkg.device_count() > 0:
        with pytest.raises(pkg.OrbxError) as e:
            pkg.update_normal_and_depth(S.NORMAL_CASES["status"]()["table"], device=pkg.device_count() + 7)
    else:
        with pytest.raises(pkg.OrbxError) as e:
            pkg.update_normal_and_depth(S.NORMAL_CASES["status"]()["table"])
    assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
