"""GPU: the C++ host classes (orb_slam2v2-1_amd/host: ORB_SLAM2::ORBextractor, ORBmatcher,
ComputeStereoMatchesHIP) called the way Frame.cc / Tracking.cc call the reference classes,
compared with the CPU oracle.  The driver is tests/cpp/host_driver.cc (compiled here with g++
against the cv/Frame shims; in the reference tree the same sources build against OpenCV)."""
import os
import subprocess

import numpy as np
import pytest

import host_cpp_cases     # the scenes tests/test_match_threads_host_cpp_gpu.py runs too

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIBDIR = os.path.join(ROOT, "orb_slam2v2-1_amd", "lib")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    import importlib
    importlib.import_module("orb_slam2v2-1_amd.build").build()
    exe = str(tmp_path_factory.mktemp("bin") / "host_driver")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"), "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "host_driver.cc"), "-L" + LIBDIR, "-lorb_host",
                           "-lorbx_hip", "-Wl,-rpath," + LIBDIR])
    return exe


def _run(exe, *args, **extra_env):
    env = dict(os.environ, **extra_env)
    # the C++ classes take their Gaussian flavour from ORBX_GAUSS_ROUNDING; a session run under another flavour (ORBX_TEST_GAUSS_FLAVOUR, the
    # harness's switch for oracle and Python wrapper) hands it on - the strings are the same
    env.setdefault("ORBX_GAUSS_ROUNDING", os.environ.get("ORBX_TEST_GAUSS_FLAVOUR", "half_up"))
    # one HIP runtime per process: the driver is a plain C++ program, it uses /opt/rocm's
    out = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, env=env, timeout=300)
    assert out.returncode == 0, out.stderr + out.stdout
    return [int(t) for t in out.stdout.split()]


def test_extractor_class(driver, oracle, synth, pkg, tmp_path):
    w, h, nf = 752, 480, 1000
    img = synth.frame(w, h, 21)
    img.tofile(tmp_path / "a.raw")
    n, pw, ph = _run(driver, "extract", tmp_path / "a.raw", w, h, nf, tmp_path / "o")
    orc = oracle.Extractor(nf, 1.2, 8, 20, 7)
    ok, od = orc.extract(img)
    k = np.fromfile(str(tmp_path / "o.kps"), pkg.KP_DTYPE)
    d = np.fromfile(str(tmp_path / "o.desc"), np.uint8).reshape(-1, 32)
    assert n == len(ok) == len(k)
    for f in ok.dtype.names:
        np.testing.assert_array_equal(k[f], ok[f], err_msg=f)
    np.testing.assert_array_equal(d, od)
    p3 = np.fromfile(str(tmp_path / "o.pyr3"), np.uint8).reshape(ph, pw)
    np.testing.assert_array_equal(p3, orc.pyramid_level(3))


@pytest.mark.parametrize("gauss", ["half_up", "sse2", "taps:56,48,34,18"])
def test_extractor_class_takes_the_flavour_from_the_environment(driver, oracle, synth, pkg, tmp_path, gauss):
    """The reference's callers construct ORBextractor with five arguments (src/Tracking.cc:119-125); a deployment selects the flavour of
    cv::GaussianBlur's column rounding with ORBX_GAUSS_ROUNDING.  A four-grey-level image (many exact rounding ties) through the C++
    class under each setting equals the oracle of that flavour, and the two oracles differ on it."""
    w, h, nf = 1241, 376, 1500
    img = ((synth.frame(w, h, 52) >> 6) * 85).astype(np.uint8)
    img.tofile(tmp_path / "a.raw")
    n, pw, ph = _run(driver, "extract", tmp_path / "a.raw", w, h, nf, tmp_path / "o", ORBX_GAUSS_ROUNDING=gauss)
    ok, od = oracle.Extractor(nf, 1.2, 8, 20, 7, gauss=gauss).extract(img)
    other = oracle.Extractor(nf, 1.2, 8, 20, 7, gauss="sse2" if gauss == "half_up" else "half_up")
    other.extract(img)
    k = np.fromfile(str(tmp_path / "o.kps"), pkg.KP_DTYPE)
    d = np.fromfile(str(tmp_path / "o.desc"), np.uint8).reshape(-1, 32)
    assert n == len(ok) == len(k)
    np.testing.assert_array_equal(k[["x", "y", "response", "octave"]], ok[["x", "y", "response", "octave"]])
    np.testing.assert_array_equal(d, od)
    ref = oracle.Extractor(nf, 1.2, 8, 20, 7, gauss=gauss)
    ref.extract(img)
    assert any((ref.blurred_level(l) != other.blurred_level(l)).any() for l in range(8)), "the test image must hold rounding ties"


def test_stereo_through_frame(driver, oracle, synth, tmp_path):
    w, h, nf = 752, 480, 1000
    l, r = synth.stereo_pair_blocky(w, h, 22)
    l.tofile(tmp_path / "l.raw"); r.tofile(tmp_path / "r.raw")
    mbf, fx = 47.9, 435.2
    N, nm = _run(driver, "stereo", tmp_path / "l.raw", tmp_path / "r.raw", w, h, nf, mbf, fx, tmp_path / "s")
    ol, orr = oracle.Extractor(nf, 1.2, 8, 20, 7), oracle.Extractor(nf, 1.2, 8, 20, 7)
    kl, dl = ol.extract(l); kr, dr = orr.extract(r)
    mb = np.float32(mbf) / np.float32(fx)
    on, our, odp = oracle.stereo_match(kl, dl, kr, dr, [ol.pyramid_level(i) for i in range(8)],
                                       [orr.pyramid_level(i) for i in range(8)], ol.scale_factors,
                                       ol.inv_scale_factors, mbf, mb)
    assert N == len(kl) and nm == on > 20
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "s.uright"), np.float32), our)
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "s.depth"), np.float32), odp)


def test_stereo_frame_in_one_call(driver, oracle, synth, pkg, tmp_path):
    """ExtractStereoFrameHIP (host/ORBmatcher.h) = the stereo Frame constructor's ExtractORB(left) || ExtractORB(right) +
    ComputeStereoMatches (src/Frame.cc:78-84, 481-655) as ONE C-ABI call (orbx_stereo_frame): both key point sets, both descriptor
    matrices, mvuRight, mvDepth and the match count equal the oracle's; the ctypes binding of the same entry point too, on a
    corner-sparse pair and with an empty image."""
    w, h, nf = 1241, 376, 2000
    l, r = synth.stereo_pair_blocky(w, h, 25)
    l.tofile(tmp_path / "l.raw"); r.tofile(tmp_path / "r.raw")
    mbf, fx = 386.1448, 718.856
    N, Nr, nm = _run(driver, "stereoframe", tmp_path / "l.raw", tmp_path / "r.raw", w, h, nf, mbf, fx, tmp_path / "f")

    def ref(l, r):
        ol, orr = oracle.Extractor(nf, 1.2, 8, 20, 7), oracle.Extractor(nf, 1.2, 8, 20, 7)
        kl, dl = ol.extract(l); kr, dr = orr.extract(r)
        mb = np.float32(mbf) / np.float32(fx)
        on, our, odp = oracle.stereo_match(kl, dl, kr, dr, [ol.pyramid_level(i) for i in range(8)],
                                           [orr.pyramid_level(i) for i in range(8)], ol.scale_factors, ol.inv_scale_factors, mbf, mb)
        return kl, dl, kr, dr, on, our, odp
    kl, dl, kr, dr, on, our, odp = ref(l, r)
    assert (N, Nr, nm) == (len(kl), len(kr), on) and on > 100
    for tag, k, d in (("", kl, dl), ("r", kr, dr)):
        g = np.fromfile(str(tmp_path / ("f.kps" + tag)), np.uint8).reshape(-1, 28)
        gk = np.frombuffer(g.tobytes(), pkg.KP_DTYPE)
        for f in ("x", "y", "size", "response", "octave", "class_id"):
            np.testing.assert_array_equal(gk[f], k[f], err_msg=tag + f)
        np.testing.assert_allclose(gk["angle"], k["angle"], atol=1e-4, rtol=0)
        np.testing.assert_array_equal(np.fromfile(str(tmp_path / ("f.desc" + tag)), np.uint8).reshape(-1, 32), d)
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "f.uright"), np.float32), our)
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "f.depth"), np.float32), odp)
    # the same entry point through ctypes, on a corner-sparse pair (levels that fall back to the exact quad-tree) ...
    ex = pkg.ORBextractor(nf, 1.2, 8, 20, 7)
    l2, r2 = synth.natural_pair(w, h, 26)
    kl, dl, kr, dr, on, our, odp = ref(l2, r2)
    for rep in range(2):
        f = ex.stereo_frame(l2, r2, mbf, float(np.float32(mbf) / np.float32(fx)))
    assert (len(f["kl"]), len(f["kr"]), f["nmatch"]) == (len(kl), len(kr), on)
    np.testing.assert_array_equal(f["kl"][["x", "y", "response", "octave"]], kl[["x", "y", "response", "octave"]])
    np.testing.assert_array_equal(f["dl"], dl)
    np.testing.assert_array_equal(f["dr"], dr)
    np.testing.assert_array_equal(f["uright"], our)
    np.testing.assert_array_equal(f["depth"], odp)
    # ... and an image without key points: zero counts, no error (a flat image has no FAST corner)
    f0 = ex.stereo_frame(np.full((h, w), 80, np.uint8), np.full((h, w), 80, np.uint8), mbf, 0.5)
    assert (len(f0["kl"]), len(f0["kr"]), f0["nmatch"]) == (0, 0, 0)


def test_search_for_initialization_through_frames(driver, oracle, synth, tmp_path):
    w, h, nf = 640, 480, 2000
    a = synth.frame(w, h, 23)
    b = np.roll(a, (2, 4), axis=(0, 1))
    a.tofile(tmp_path / "a.raw"); b.tofile(tmp_path / "b.raw")
    n1, n2, nm = _run(driver, "init", tmp_path / "a.raw", tmp_path / "b.raw", w, h, nf, tmp_path / "i")
    orc = oracle.Extractor(nf, 1.2, 8, 20, 7)
    k1, d1 = orc.extract(a)
    k2, d2 = orc.extract(b)
    prev = np.stack([k1["x"], k1["y"]], 1)
    on, om12, oprev = oracle.search_for_initialization(k1, d1, k2, d2, oracle.grid_geom(w, h), prev, 100, 0.9, True)
    assert (n1, n2) == (len(k1), len(k2)) and nm == on > 30
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "i.m12"), np.int32), om12)
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "i.prev"), np.float32).reshape(-1, 2), oprev)


def test_search_by_projection_through_mappoints(driver, oracle, synth, tmp_path):
    w, h, nf = 1241, 376, 1000
    img = synth.frame(w, h, 24)
    img.tofile(tmp_path / "a.raw")
    orc = oracle.Extractor(nf, 1.2, 8, 20, 7)
    k, d = orc.extract(img)
    rng = np.random.default_rng(3)
    m = 1200
    idx = rng.choice(len(k), m, replace=True)
    mps = np.zeros(m, oracle.MP_DTYPE)
    mps["in_view"] = rng.random(m) > 0.1
    mps["proj_x"] = k["x"][idx] + rng.normal(0, 1.5, m)
    mps["proj_y"] = k["y"][idx] + rng.normal(0, 1.5, m)
    mps["proj_xr"] = mps["proj_x"] - 5
    mps["level"] = np.clip(k["octave"][idx] + rng.integers(-1, 2, m), 0, 7)
    mps["view_cos"] = rng.uniform(0.99, 1.0, m)
    mps["observations"] = rng.integers(0, 4, m)
    md = d[idx] ^ (rng.integers(0, 256, (m, 32), dtype=np.uint8) & rng.integers(0, 256, (m, 32), dtype=np.uint8) &
                   rng.integers(0, 256, (m, 32), dtype=np.uint8))
    mps.tofile(tmp_path / "mps.bin"); md.tofile(tmp_path / "md.bin")
    N, nm = _run(driver, "projmp", tmp_path / "a.raw", w, h, nf, tmp_path / "mps.bin", tmp_path / "md.bin", tmp_path / "p")
    on, ofm = oracle.search_by_projection_mp(k, d, np.full(len(k), -1, np.float32), oracle.grid_geom(w, h),
                                             orc.scale_factors, mps, md, np.full(len(k), -1, np.int32), None, 3.0, 0.8)
    assert N == len(k) and nm == on > 100
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "p.held"), np.int32), ofm)


def test_search_by_projection_through_keyframe(driver, oracle, synth, tmp_path):
    """SURVEY §8(f) rank 1 through the C++ class: ORBmatcher::SearchByProjection(Frame&, KeyFrame*,
    sAlreadyFound, th, ORBdist) — projection + PredictScale on the host, matching on the GPU."""
    w, h, nf = 1241, 376, 1000
    img = synth.frame(w, h, 25)
    img.tofile(tmp_path / "a.raw")
    orc = oracle.Extractor(nf, 1.2, 8, 20, 7)
    k, d = orc.extract(img)
    sf = orc.scale_factors
    rng = np.random.default_rng(5)
    fx, fy, cx, cy = 718.856, 718.856, 607.19, 185.2
    m = 1300
    idx = rng.choice(len(k), m, replace=True)
    z = rng.uniform(4, 40, m).astype(np.float32)
    kf = np.zeros(m, oracle.KFPOINT_DTYPE)
    kf["valid"] = rng.random(m) > 0.2
    kf["wx"] = ((k["x"][idx] + rng.normal(0, 2, m) - cx) / fx * z).astype(np.float32)
    kf["wy"] = ((k["y"][idx] + rng.normal(0, 2, m) - cy) / fy * z).astype(np.float32)
    kf["wz"] = z
    kf["max_distance"] = z * sf[k["octave"][idx]] * rng.uniform(0.85, 1.15, m)
    kf["min_distance"] = kf["max_distance"] / sf[7] * rng.uniform(0.5, 1.0, m)
    kf["angle"] = (k["angle"][idx] + rng.normal(0, 5, m)) % 360
    kd = d[idx] ^ (rng.integers(0, 256, (m, 32), dtype=np.uint8) & rng.integers(0, 256, (m, 32), dtype=np.uint8) &
                   rng.integers(0, 256, (m, 32), dtype=np.uint8))
    kf.tofile(tmp_path / "kf.bin"); kd.tofile(tmp_path / "kd.bin")
    th, orbdist, tx, tz = 10.0, 100, 0.03, 0.2
    N, nm = _run(driver, "projkf", tmp_path / "a.raw", w, h, nf, tmp_path / "kf.bin", tmp_path / "kd.bin", th, orbdist,
                 "%r,%r,%r,%r" % (fx, fy, cx, cy), "%r,%r" % (tx, tz), tmp_path / "k")
    Tc = np.eye(4, dtype=np.float32)
    Tc[0, 3], Tc[2, 3] = tx, tz
    cam = oracle.Cam(fx, fy, cx, cy, 0.0, 0.0)
    log_sf = np.float32(np.log(np.float32(1.2)))
    on, ocm = oracle.search_by_projection_kf(k, d, oracle.grid_geom(w, h), sf, log_sf, cam, Tc, kf, kd,
                                             np.full(len(k), -1, np.int32), th, orbdist)
    assert N == len(k) and nm == on > 100
    np.testing.assert_array_equal(np.fromfile(str(tmp_path / "k.held"), np.int32), ocm)


# ---- KeyFrame-side matchers through the C++ classes
def _kf_setup(oracle, synth, seed, distorted, tmp_path, m=1500):
    import kf_scene as ks
    w, h, nf = 1241, 376, 1000
    rng = np.random.default_rng(seed)
    img = synth.frame(w, h, 40 + seed)
    img.tofile(tmp_path / "kf.raw")
    orc = oracle.Extractor(nf, 1.2, 8, 20, 7)
    k, d = orc.extract(img)
    sf = orc.scale_factors
    cam = oracle.Cam(ks.FX, ks.FY, ks.CX, ks.CY, ks.MBF, np.float32(ks.MBF) / np.float32(ks.FX))
    g, ga, b = ks.geoms(oracle, w, h, distorted)
    args = dict(w=w, h=h, nf=nf, bounds="%r,%r,%r,%r" % tuple(float(v) for v in b),
                cam="%r,%r,%r,%r,%r" % (ks.FX, ks.FY, ks.CX, ks.CY, ks.MBF))
    return ks, rng, k, d, sf, cam, np.float32(np.log(np.float32(1.2))), g, ga, args, m


def _kf_run(driver, sub, tmp_path, args, pts, pd, aux, th):
    pts.tofile(tmp_path / "pts.bin"); pd.tofile(tmp_path / "pd.bin")
    with open(tmp_path / "aux.bin", "wb") as f:
        for a in aux:
            f.write(np.ascontiguousarray(a).tobytes())
    n, ret = _run(driver, "kf", sub, tmp_path / "kf.raw", args["w"], args["h"], args["nf"], args["bounds"], args["cam"],
                  tmp_path / "pts.bin", tmp_path / "pd.bin", tmp_path / "aux.bin", th, tmp_path / "o")
    return n, ret, np.fromfile(str(tmp_path / "o.i32"), np.int32)


@pytest.mark.parametrize("distorted", [False, True])
def test_search_by_projection_sim3_class(driver, oracle, synth, tmp_path, distorted):
    """ORBmatcher::SearchByProjection(KeyFrame*, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:290-403)."""
    ks, rng, k, d, sf, cam, log_sf, g, ga, args, m = _kf_setup(oracle, synth, 1, distorted, tmp_path)
    S = ks.pose(rng, scale=0.93)
    pts, pd, _ = ks.points_for(oracle, rng, k, d, sf, S, m, scale=0.93)
    pts["valid"] = rng.random(m) > 0.1          # invalid -> the driver marks the point bad
    matched = np.full(len(k), -1, np.int32)
    matched[rng.choice(len(k), 50, replace=False)] = -2
    on, om = oracle.search_by_projection_sim3(k, d, g, sf, log_sf, cam, S, pts, pd, matched, 10, ga)
    n, ret, res = _kf_run(driver, "projsim3", tmp_path, args, pts, pd, [S, matched], 10)
    assert n == len(k) and on > 200
    assert ret == on
    np.testing.assert_array_equal(res, om)


@pytest.mark.parametrize("distorted", [False, True])
def test_fuse_class(driver, oracle, synth, tmp_path, distorted):
    """ORBmatcher::Fuse(KeyFrame*, vpMapPoints, th) (src/ORBmatcher.cc:827-977): GPU window search with the
    stereo / mono reprojection gate + the reference's replace / add bookkeeping on the host."""
    ks, rng, k, d, sf, cam, log_sf, g, ga, args, m = _kf_setup(oracle, synth, 2, distorted, tmp_path)
    n = len(k)
    T = ks.pose(rng)
    pts, pd, _ = ks.points_for(oracle, rng, k, d, sf, T, m)
    isnull = (rng.random(m) < 0.05).astype(np.int32)
    pts["valid"] = 1 - isnull
    bad, in_kf, obs, slot, ext_obs, ext_bad = ks.fuse_state(rng, n, m)
    uright = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 30, n), -1).astype(np.float32)
    inv_s2 = (np.float32(1.0) / (sf * sf)).astype(np.float32)
    on, obi, oact, st = oracle.fuse(k, d, uright, g, sf, inv_s2, log_sf, cam, T, pts, pd, bad, in_kf, obs, slot, ext_obs,
                                    ext_bad, 3.0, ga)
    assert on > 200 and all((oact == a).sum() > 0 for a in (1, 2, 3, 4))
    nk, ret, res = _kf_run(driver, "fuse", tmp_path, args, pts, pd, [T, uright, slot, ext_obs, ext_bad, bad, obs, isnull], 3.0)
    assert nk == n and ret == on
    o = np.split(res, np.cumsum([n, n, m, m, m]))
    np.testing.assert_array_equal(o[0], st["slot"])
    np.testing.assert_array_equal(o[1][slot == -2], st["ext_bad"][slot == -2])
    np.testing.assert_array_equal(o[2], st["bad"])
    np.testing.assert_array_equal(o[3], st["in_kf"])
    np.testing.assert_array_equal(o[4], st["obs"])


def test_fuse_sim3_class(driver, oracle, synth, tmp_path):
    """ORBmatcher::Fuse(KeyFrame*, Scw, vpPoints, th, vpReplacePoint) (src/ORBmatcher.cc:979-1102)."""
    ks, rng, k, d, sf, cam, log_sf, g, ga, args, m = _kf_setup(oracle, synth, 3, True, tmp_path)
    n = len(k)
    S = ks.pose(rng, scale=1.11)
    pts, pd, _ = ks.points_for(oracle, rng, k, d, sf, S, m, scale=1.11)
    bad, in_kf, obs, slot, ext_obs, ext_bad = ks.fuse_state(rng, n, m)
    pts["valid"] = (bad == 0) & ~((in_kf == 1) & (bad == 0))     # !isBad && !spAlreadyFound.count(pMP)
    on, obi, orep, oslot = oracle.fuse_sim3(k, d, g, sf, log_sf, cam, S, pts, pd, bad, slot, ext_bad, 4.0, ga)
    assert on > 200 and (orep >= 0).sum() > 0 and (orep == -2).sum() > 0 and (oslot != slot).sum() > 0
    uright = np.full(n, -1, np.float32)
    nk, ret, res = _kf_run(driver, "fusesim3", tmp_path, args, pts, pd,
                           [S, uright, slot, ext_obs, ext_bad, bad, obs, np.zeros(m, np.int32)], 4.0)
    assert nk == n and ret == on
    o = np.split(res, np.cumsum([n, n, m, m, m]))
    np.testing.assert_array_equal(o[0], oslot)
    np.testing.assert_array_equal(o[5], orep)


def test_search_by_sim3_class(driver, oracle, synth, tmp_path):
    """ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1104-1328): two keyframes, mutual window search."""
    import kf_scene as ks
    w, h, nf = 1241, 376, 1000
    rng = np.random.default_rng(5)
    img = synth.frame(w, h, 46)
    img.tofile(tmp_path / "a.raw")
    orc = oracle.Extractor(nf, 1.2, 8, 20, 7)
    k, d = orc.extract(img)
    n = len(k)
    sf = orc.scale_factors
    log_sf = np.float32(np.log(np.float32(1.2)))
    cam = oracle.Cam(ks.FX, ks.FY, ks.CX, ks.CY, ks.MBF, np.float32(ks.MBF) / np.float32(ks.FX))
    g, ga, b = ks.geoms(oracle, w, h, True)
    # world = camera 1 up to a small pose; camera 2 = slightly moved; p1 = s12*R12*p2 + t12
    T1 = ks.pose(rng).astype(np.float64)
    D = np.eye(4); D[:3, :3] = ks.rot(*rng.normal(0, 0.002, 3)); D[:3, 3] = rng.normal(0, 0.02, 3)
    T2 = D @ T1
    s12 = np.float32(1.03)
    R12 = D[:3, :3].T
    t12 = -R12 @ D[:3, 3]
    T1f, T2f, R12f, t12f = [np.ascontiguousarray(a, np.float32) for a in (T1, T2, R12, t12)]

    def slot_points(T):
        z = rng.uniform(4, 40, n)
        pc = np.stack([(k["x"] + rng.normal(0, 1, n) - ks.CX) / ks.FX * z, (k["y"] + rng.normal(0, 1, n) - ks.CY) / ks.FY * z, z], 1)
        pw = (pc - T[:3, 3]) @ T[:3, :3]
        p = np.zeros(n, oracle.MP3D_DTYPE)
        p["wx"], p["wy"], p["wz"] = pw[:, 0], pw[:, 1], pw[:, 2]
        p["max_distance"] = z * sf[k["octave"]] * rng.uniform(0.9, 1.1, n)
        p["min_distance"] = p["max_distance"] / sf[7] * rng.uniform(0.5, 1.0, n)
        r = rng.random(n)
        p["valid"] = np.where(r < 0.15, 0, np.where(r < 0.22, 2, 1))      # no point / bad point / good point
        flips = rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8) & \
            rng.integers(0, 256, (n, 32), dtype=np.uint8)
        return p, d ^ flips
    p1, pd1 = slot_points(T1)
    p2, pd2 = slot_points(T2)
    pre = np.full(n, -1, np.int32)
    cand = np.flatnonzero(p2["valid"] == 1)
    pick = rng.choice(n, 40, replace=False)
    pre[pick] = rng.choice(cand, 40, replace=False)
    # the flat "valid" of the oracle: point present, not already matched, not bad (:1134-1158, :1234-1238)
    already1 = pre >= 0
    already2 = np.zeros(n, bool); already2[pre[pre >= 0]] = True
    o1 = p1.copy(); o1["valid"] = (p1["valid"] == 1) & ~already1
    o2 = p2.copy(); o2["valid"] = (p2["valid"] == 1) & ~already2
    on, om12 = oracle.search_by_sim3(k, d, k, d, g, sf, log_sf, cam, T1f, T2f, s12, R12f, t12f, o1, pd1, o2, pd2, 7.5, ga)
    assert on > 200
    p1.tofile(tmp_path / "p1.bin"); pd1.tofile(tmp_path / "d1.bin"); p2.tofile(tmp_path / "p2.bin"); pd2.tofile(tmp_path / "d2.bin")
    with open(tmp_path / "aux.bin", "wb") as f:
        for a in (T1f, T2f, np.array([s12], np.float32), R12f, t12f, pre):
            f.write(np.ascontiguousarray(a).tobytes())
    bounds = "%r,%r,%r,%r" % tuple(float(v) for v in b)
    camarg = "%r,%r,%r,%r,%r" % (ks.FX, ks.FY, ks.CX, ks.CY, ks.MBF)
    n1, n2, ret = _run(driver, "sim3", tmp_path / "a.raw", tmp_path / "a.raw", w, h, nf, bounds, camarg, tmp_path / "p1.bin",
                       tmp_path / "d1.bin", tmp_path / "p2.bin", tmp_path / "d2.bin", tmp_path / "aux.bin", 7.5, tmp_path / "o")
    assert n1 == n2 == n and ret == on
    res = np.fromfile(str(tmp_path / "o.i32"), np.int32)
    expect = np.where(om12 >= 0, om12, pre)
    np.testing.assert_array_equal(res, expect)


def test_compute_distinctive_descriptors_batched(driver, oracle, tmp_path):
    """MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:252-317) for a batch of map points through
    the C++ gather (observations in std::map order, bad keyframes and bad points skipped)."""
    rng = np.random.default_rng(9)
    sizes = [0, 1, 2, 5, 64, 65, 130] + list(rng.integers(1, 30, 60))
    blocks, offsets = [], [0]
    for n in sizes:
        base = rng.integers(0, 256, 32, dtype=np.uint8)
        d = base[None, :] ^ (rng.integers(0, 256, (n, 32), dtype=np.uint8) & rng.integers(0, 256, (n, 32), dtype=np.uint8) & np.uint8(0x33))
        blocks.append(d)
        offsets.append(offsets[-1] + n)
    np.array(offsets, np.int32).tofile(tmp_path / "off.bin")
    np.concatenate(blocks).tofile(tmp_path / "desc.bin")
    badkf = 3
    m, n = _run(driver, "distinct", tmp_path / "off.bin", tmp_path / "desc.bin", badkf, tmp_path / "o")
    res = np.fromfile(str(tmp_path / "o.best"), np.uint8).reshape(m, 33)
    expect_n = 0
    for p, d in enumerate(blocks):
        rows = np.delete(d, badkf, axis=0) if len(d) > badkf else d        # keyframe 3 is bad: its row is skipped
        if p % 11 == 10 or len(rows) == 0:
            assert res[p, 0] == 0
            continue
        oi, _ = oracle.distinctive_descriptor(rows)
        assert res[p, 0] == 1
        np.testing.assert_array_equal(res[p, 1:], rows[oi], err_msg=str(p))
        expect_n += 1
    assert m == len(sizes) and n == expect_n > 40


def test_search_local_points_class(driver, oracle, synth, tmp_path):
    """Tracking::SearchLocalPoints' projection loop + SearchByProjection (src/Tracking.cc:1305-1339,
    src/Frame.cc:284-340) through SearchLocalPointsHIP: one fused GPU call."""
    args, check = host_cpp_cases.local_points_case(oracle, synth, tmp_path)
    check(_run(driver, "local", *args, tmp_path / "o"), tmp_path / "o")


def test_bow_classes(driver, oracle, tmp_path):
    """ORBVocabulary::loadFromTextFile / transform (Frame::ComputeBoW, KeyFrame::ComputeBoW) and both
    ORBmatcher::SearchByBoW overloads through the C++ classes, against the DBoW2 / ORBmatcher restatement."""
    args, check = host_cpp_cases.bow_case(oracle, tmp_path)
    check(_run(driver, "bow", *args, tmp_path / "o"), tmp_path / "o")


@pytest.mark.parametrize("only_stereo", [0, 1])
def test_search_for_triangulation_class(driver, oracle, tmp_path, only_stereo):
    """ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-825) through the C++ class: epipole from the two
    keyframe poses, flags from map points / mvuRight / bOnlyStereo, pairs in increasing first index."""
    args, check = host_cpp_cases.triangulation_case(oracle, tmp_path, only_stereo)
    check(_run(driver, "tri", *args, tmp_path / "o"), tmp_path / "o")
