"""The matchers at every size-chosen path, bit for bit against the CPU oracle.

The guided searches (orbx_match_fast.hip, orbx_match.hip) pick a resolver by size - the whole-workgroup fixed point k_resolve_par with
2 or 4 queries per thread, the single-wave speculative resolvers, or the exact one-workgroup kernels - and fall back to the exact
kernels on several conditions; the stereo matcher moves its SAD median out of LDS, widens its row bins and restarts a full candidate
list.  Results never depend on the path, so every case here also asks the developer build which path ran (orbm_debug_match_path /
orbm_debug_resolve_plan / orbm_debug_stereo_path, include/orbx_dev.h): the cases on the two sides of a threshold are shown to run
different code.  Inputs are keypoints the extractor really produces (replicated, jittered, with sparse bit flips in the copied
descriptors), kept inside the domain src/Frame.cc defines."""
import numpy as np
import pytest

# the builders live in tests/match_cases.py: the threaded worker (tests/match_threads_worker.py) builds its regrow cases with them
from match_cases import (limits_frame, flips as _flips, kps as _kps, cluster as _cluster, init_inputs, cand_cap_init_inputs)

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
FX, FY, CX, CY, MBF = 1000.0, 1000.0, 960.0, 540.0, 400.0
RP_T, QK, CAND_CAP = 1024, 8, 512
MODE_MP, MODE_FRAME, MODE_WIN, MODE_INIT = 0, 1, 2, 3


@pytest.fixture(autouse=True)
def dev_matchers(pkg, hooks):
    """Every matcher call of this module runs in the developer build (the path hooks read its per-thread record), with the default
    resolver options of that library."""
    L = pkg.matcher_lib()
    assert L._orbx_developer
    L.orbm_set_thread_option(2, 0)
    L.orbm_set_thread_option(3, 0)
    yield L
    L.orbm_set_thread_option(2, 0)
    L.orbm_set_thread_option(3, 0)


@pytest.fixture(scope="module")
def frame(oracle, synth):
    """One 1920x1080 / 4000-feature extraction (the oracle's: bit-identical to the HIP extractor, tested elsewhere)."""
    return limits_frame(oracle, synth)


def _path(pkg):
    return pkg.debug_match_path()


def _plan(pkg, mode, m, n):
    return pkg.debug_resolve_plan(mode, m, n)


# ---------------------------------------------------------------------------------------------------------------------------------
# the resolver's LDS budget, no launches

def _par_lds(m, n):
    n = np.asarray(n, np.int64)
    q = 2 if m <= 2 * RP_T else 4
    return 4 * (QK * RP_T * q + 2 * n + (n + 31) // 32)


def _old_rule_windows(pkg, mode, m):
    """The n for which the former hard-coded rule (dynamic LDS <= 158 KiB) chose k_resolve_par although dynamic + static LDS of that
    instance passes the device's per-workgroup limit."""
    _, _, stat, limit = _plan(pkg, mode, m, 0)
    n = np.arange(30001)
    lds = _par_lds(m, n)
    return n[(lds <= 158 * 1024) & (lds + stat > limit)]


def test_resolve_plan_sweep_fits_the_device(pkg):
    """Every mode, m in {1, 2048, 2049, 4096, 4097} and every n from 0 to 30001: when the plan picks k_resolve_par, its dynamic plus
    static LDS fits the device's per-workgroup limit, and it is picked whenever it fits (m <= 4096, n <= 30000)."""
    for mode in (MODE_MP, MODE_FRAME, MODE_WIN):
        for m in (1, 2048, 2049, 4096, 4097):
            res = np.zeros(30002, np.int64)
            lds = np.zeros(30002, np.int64)
            stat = np.zeros(30002, np.int64)
            for n in range(30002):
                res[n], lds[n], stat[n], limit = _plan(pkg, mode, m, n)
            assert limit >= 64 * 1024
            n = np.arange(30002)
            par = (res == pkg.RES_PAR_Q2) | (res == pkg.RES_PAR_Q4)
            over = par & (lds + stat > limit)
            assert not over.any(), "mode %d m %d: k_resolve_par over the LDS limit at n = %s" % (mode, m, n[over][:20])
            assert (res[30001] == pkg.RES_EXACT) and not (res[:30001] == pkg.RES_EXACT).any()
            want_q = pkg.RES_PAR_Q2 if m <= 2048 else pkg.RES_PAR_Q4
            assert set(np.unique(res[par])) <= {want_q}
            if m > 4096:
                assert not par.any()
            else:
                _, _, stat_q, _ = _plan(pkg, mode, m, 0)
                fits = _par_lds(m, n[:30001]) + stat_q <= limit
                np.testing.assert_array_equal(par[:30001], fits)
            wave = res[:30001] == pkg.RES_WAVE
            np.testing.assert_array_equal(lds[:30001][wave], 2 * ((n[:30001][wave] + 15) & ~15))
    # SearchForInitialization: k_resolve_init's LDS plan up to n2 = 7000, then the exact kernel
    for n in (0, 1, 6999, 7000, 7001, 30000):
        res, lds, stat, limit = _plan(pkg, MODE_INIT, 2000, n)
        if n <= 7000:
            assert res == pkg.RES_WAVE and lds == 8 * n + ((n + 15) & ~15) and lds + stat <= limit
        else:
            assert res == pkg.RES_EXACT
    assert _plan(pkg, MODE_INIT, 65536, 100)[0] == pkg.RES_EXACT


def test_former_lds_windows_take_the_single_wave_resolver(pkg):
    """The windows in which the former 158-KiB rule launched k_resolve_par over the limit: with the budget computed from the device
    limit and each instance's static LDS, their every n plans the single-wave resolver."""
    found = {}
    for mode in (MODE_MP, MODE_FRAME, MODE_WIN):
        for m in (2048, 4096):
            win = _old_rule_windows(pkg, mode, m)
            found[(mode, m)] = (int(win[0]), int(win[-1])) if len(win) else None
            for n in win:
                assert _plan(pkg, mode, m, int(n))[0] == pkg.RES_WAVE
    print("former over-budget windows (mode, m) -> (first n, last n):", found)


# ---------------------------------------------------------------------------------------------------------------------------------
# guided searches: the three modes at a size, against the oracle

def _mappoints(k, d, rng, m, spread=1.5):
    idx = rng.choice(len(k), size=m, replace=len(k) < m)
    mps = np.zeros(m, [("in_view", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("level", "<i4"),
                       ("view_cos", "<f4"), ("observations", "<i4")])
    mps["in_view"] = rng.random(m) > 0.1
    mps["proj_x"] = k["x"][idx] + rng.normal(0, spread, m)
    mps["proj_y"] = k["y"][idx] + rng.normal(0, spread, m)
    mps["proj_xr"] = mps["proj_x"] - rng.uniform(1, 30, m)
    mps["level"] = np.clip(k["octave"][idx] + rng.integers(-1, 2, m), 0, 7)
    mps["view_cos"] = rng.uniform(0.99, 1.0, m)
    mps["observations"] = rng.integers(0, 4, m)
    return mps, d[idx] ^ _flips(rng, (m, 32))


def _presets(rng, n, m, count=120):
    """Holders set before the call: -2 (another map point, ext_obs observations) and this call's map points, on both ends of the
    keypoint range (the resolver reads the holders past RP_Q * RP_T in a tail loop)."""
    fm = np.full(n, -1, np.int32)
    ext = np.zeros(n, np.int32)
    c = min(count, n)
    pre = np.unique(np.concatenate([rng.choice(n, c, replace=False), np.arange(max(0, n - 8), n)]))
    fm[pre] = -2
    ext[pre] = rng.integers(0, 3, len(pre))
    own = pre[::3]
    fm[own] = rng.integers(0, m, len(own))
    return fm, ext


def run_mp(pkg, oracle, frame, n, m, seed, th=3.0, ratio=0.8, kd=None, mps=None, presets=True):
    rng = np.random.default_rng(seed)
    k, d = kd if kd is not None else _kps(frame, n, rng)
    sf = frame[2]
    if mps is None:
        mps = _mappoints(k, d, rng, m)
    if presets:
        uright = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 30, n), -1).astype(np.float32)
        fm, ext = _presets(rng, n, m)
    else:
        uright, fm, ext = np.full(n, -1, np.float32), np.full(n, -1, np.int32), None
    on, ofm = oracle.search_by_projection_mp(k, d, uright, oracle.grid_geom(W, H), sf, mps[0], mps[1], fm, ext, th, ratio)
    gn, gfm = pkg.ORBmatcher(ratio, True).SearchByProjection(k, d, uright, pkg.grid_geom(W, H), sf, mps[0], mps[1], fm, ext, th)
    assert gn == on, (n, m, gn, on, _path(pkg))
    np.testing.assert_array_equal(gfm, ofm)
    return _path(pkg), on


def run_frame(pkg, oracle, frame, n, m, seed, mono=False, dz=0.5):
    rng = np.random.default_rng(seed)
    k, d = _kps(frame, n, rng)
    sf = frame[2]
    cam_o = oracle.Cam(FX, FY, CX, CY, MBF, np.float32(MBF) / np.float32(FX))
    cam_g = pkg.Camera(FX, FY, CX, CY, MBF, np.float32(MBF) / np.float32(FX))
    idx = rng.choice(n, m, replace=n < m)
    z = rng.uniform(4, 40, m).astype(np.float32)
    last = np.zeros(m, oracle.LASTPT_DTYPE)
    last["has_mp"] = rng.random(m) > 0.2
    last["wx"] = (k["x"][idx] + rng.normal(0, 1.0, m) - CX) / FX * z
    last["wy"] = (k["y"][idx] + rng.normal(0, 1.0, m) - CY) / FY * z
    last["wz"] = z
    last["observations"] = rng.integers(0, 3, m)
    last["octave"] = k["octave"][idx]
    last["angle"] = (k["angle"][idx] + rng.normal(0, 4, m)) % 360
    ld = d[idx] ^ _flips(rng, (m, 32), 3)
    Tc = np.eye(4, dtype=np.float32)
    Tc[0, 3] = 0.01
    Tl = np.eye(4, dtype=np.float32)
    Tl[2, 3] = dz
    uright = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 30, n), -1).astype(np.float32)
    cur, ext = _presets(rng, n, m)
    on, ocm = oracle.search_by_projection_frame(k, d, uright, oracle.grid_geom(W, H), sf, cam_o, Tc, Tl, last, ld, cur, ext, 7.0,
                                                mono, True)
    gn, gcm = pkg.ORBmatcher(0.9, True).SearchByProjectionFrame(k, d, uright, pkg.grid_geom(W, H), sf, cam_g, Tc, Tl, last, ld, cur,
                                                                ext, 7.0, mono)
    assert gn == on, (n, m, gn, on, _path(pkg))
    np.testing.assert_array_equal(gcm, ocm)
    return _path(pkg), on


def run_win(pkg, oracle, frame, n, m, seed, th=3.0, orbdist=100):
    """The projected-window matcher as SearchByProjection(Frame&, KeyFrame*, ...) uses it (host projection + orbm_match_windows)."""
    rng = np.random.default_rng(seed)
    k, d = _kps(frame, n, rng)
    sf = frame[2]
    cam = oracle.Cam(FX, FY, CX, CY, MBF, np.float32(MBF) / np.float32(FX))
    idx = rng.choice(n, m, replace=n < m)
    z = rng.uniform(4, 40, m).astype(np.float32)
    kf = np.zeros(m, oracle.KFPOINT_DTYPE)
    kf["valid"] = rng.random(m) > 0.15
    kf["wx"] = (k["x"][idx] + rng.normal(0, 1.5, m) - CX) / FX * z
    kf["wy"] = (k["y"][idx] + rng.normal(0, 1.5, m) - CY) / FY * z
    kf["wz"] = z
    lvl = k["octave"][idx]
    kf["max_distance"] = z * sf[lvl] * rng.uniform(0.85, 1.15, m)
    kf["min_distance"] = kf["max_distance"] / sf[7] * rng.uniform(0.5, 1.0, m)
    kf["angle"] = (k["angle"][idx] + rng.normal(0, 5, m)) % 360
    kd = d[idx] ^ _flips(rng, (m, 32), 3)
    Tc = np.eye(4, dtype=np.float32)
    Tc[0, 3], Tc[2, 3] = 0.002, 0.01
    cur = np.full(n, -1, np.int32)
    pre = np.unique(np.concatenate([rng.choice(n, min(60, n), replace=False), np.arange(max(0, n - 8), n)]))
    cur[pre] = -2
    log_sf = np.float32(np.log(np.float32(1.2)))
    on, ocm = oracle.search_by_projection_kf(k, d, oracle.grid_geom(W, H), sf, log_sf, cam, Tc, kf, kd, cur, th, orbdist)
    q = oracle.kf_window_queries(kf, oracle.grid_geom(W, H), sf, log_sf, cam, Tc, th)
    gn, gcm = pkg.match_windows(k, d, None, pkg.grid_geom(W, H), q, kd, cur, None, orbdist, True)
    assert gn == on, (n, m, gn, on, _path(pkg))
    np.testing.assert_array_equal(gcm, ocm)
    return _path(pkg), on


RUN = {MODE_MP: run_mp, MODE_FRAME: run_frame, MODE_WIN: run_win}


def _expect(pkg, mode, m, n, path):
    """The path of a call that did not fall back for its candidates: what the plan says, no fall-back."""
    res, lds, _, _ = _plan(pkg, mode, m, n)
    assert path == (res, pkg.FB_NONE, lds), (mode, m, n, path, res, lds)
    return res


@pytest.mark.parametrize("m,want", [(2048, "q2"), (2049, "q4"), (4096, "q4"), (4097, "wave")])
def test_queries_threshold_mappoints(pkg, oracle, frame, m, want):
    """m = 2048 / 2049 (RP_Q 2 -> 4) and 4096 / 4097 (-> the single-wave resolver), SearchByProjection(F, MPs)."""
    path, on = run_mp(pkg, oracle, frame, 3000, m, 100 + m)
    assert on > 300
    res = _expect(pkg, MODE_MP, m, 3000, path)
    assert res == {"q2": pkg.RES_PAR_Q2, "q4": pkg.RES_PAR_Q4, "wave": pkg.RES_WAVE}[want]


@pytest.mark.parametrize("mode", [MODE_FRAME, MODE_WIN])
@pytest.mark.parametrize("m", [2048, 2049, 4097])
def test_queries_threshold_frame_windows(pkg, oracle, frame, mode, m):
    path, on = RUN[mode](pkg, oracle, frame, 3000, m, 200 + m + mode)
    assert on > 200
    res = _expect(pkg, mode, m, 3000, path)
    assert res == (pkg.RES_PAR_Q2 if m <= 2048 else pkg.RES_PAR_Q4 if m <= 4096 else pkg.RES_WAVE)


@pytest.mark.parametrize("mode", [MODE_MP, MODE_FRAME, MODE_WIN])
@pytest.mark.parametrize("n,m", [(2048, 1500), (2049, 1500), (4096, 2000), (4097, 2000), (3700, 3000), (4096, 3000), (4097, 3000)])
def test_keypoints_tail_threshold(pkg, oracle, frame, mode, n, m):
    """n = 2048 / 2049 (queries <= 2048: RP_Q = 2): holders of keypoints past RP_Q * RP_T are read by the resolver's tail loop, not
    from its prefetched registers; preset holders sit at the very end of the range.  With RP_Q = 4 (2048 < m <= 4096) the tail
    starts at n = 4096, where k_resolve_par<*, 4> no longer fits the LDS (from n = 3762 / 3764 on): 4096 / 4097 take the single-wave
    resolver, 3700 still the fixed point."""
    path, on = RUN[mode](pkg, oracle, frame, n, m, 300 + n + mode)
    assert on > 200
    res = _expect(pkg, mode, m, n, path)
    assert res == (pkg.RES_PAR_Q2 if m <= 2048 else pkg.RES_PAR_Q4 if n < 3762 else pkg.RES_WAVE)


def _window_edges(pkg, mode, m):
    win = _old_rule_windows(pkg, mode, m)
    if len(win):
        lo, hi = int(win[0]), int(win[-1])
    else:   # (another device limit: the edges of k_resolve_par's own budget)
        fits = [n for n in range(0, 30001, 1) if _plan(pkg, mode, m, n)[0] != pkg.RES_WAVE]
        lo = hi = fits[-1] + 1
    return sorted({lo - 1, lo, hi, hi + 1})


@pytest.mark.parametrize("mode", [MODE_MP, MODE_FRAME, MODE_WIN])
@pytest.mark.parametrize("m", [2000, 2500])
def test_lds_window_edges(pkg, oracle, frame, mode, m):
    """Both windows in which the former rule overran the LDS limit: their first and last n and one n on each side.  Inside, the
    single-wave resolver runs (no launch is refused, nothing fails); outside, k_resolve_par - either way the oracle's result."""
    seen = set()
    for n in _window_edges(pkg, mode, m):
        path, on = RUN[mode](pkg, oracle, frame, n, m, 400 + n + mode)
        assert on > 200
        seen.add(_expect(pkg, mode, m, n, path))
    assert pkg.RES_WAVE in seen and seen & {pkg.RES_PAR_Q2, pkg.RES_PAR_Q4}


def test_keypoints_30000_30001(pkg, oracle, frame):
    """n = 30000 (the fast path, single-wave resolver) / 30001 (fast -> exact), every mode."""
    for mode, m in ((MODE_MP, 2000), (MODE_FRAME, 2000), (MODE_WIN, 2000)):
        for n in (30000, 30001):
            path, on = RUN[mode](pkg, oracle, frame, n, m, 500 + n + mode)
            assert on > 200
            if n == 30000:
                _expect(pkg, mode, m, n, path)
            else:
                assert path == (pkg.RES_EXACT, pkg.FB_N, 0), path


def test_search_local_points_30001_writes_projections(pkg, oracle, frame):
    """orbm_search_local_points at n = 30001: the projections go out before the fall-back is reported, and the exact kernel's
    result is the oracle's."""
    rng = np.random.default_rng(31)
    n, m = 30001, 2500
    k, d = _kps(frame, n, rng)
    sf = frame[2]
    log_sf = np.float32(np.log(np.float32(1.2)))
    cam = oracle.Cam(FX, FY, CX, CY, MBF, np.float32(MBF) / np.float32(FX))
    pcam = pkg.Camera(FX, FY, CX, CY, MBF, np.float32(MBF) / np.float32(FX))
    idx = rng.choice(len(frame[0]), m, replace=False)
    z = rng.uniform(4, 40, m).astype(np.float32)
    pts = np.zeros(m, oracle.MP3D_DTYPE)
    pts["valid"] = rng.random(m) > 0.1
    pts["wx"] = (k["x"][idx] + rng.normal(0, 1.0, m) - CX) / FX * z
    pts["wy"] = (k["y"][idx] + rng.normal(0, 1.0, m) - CY) / FY * z
    pts["wz"] = z
    nv = np.stack([pts["wx"], pts["wy"], pts["wz"]], 1).astype(np.float64)
    dist = np.linalg.norm(nv, axis=1)
    nv /= dist[:, None]
    pts["nx"], pts["ny"], pts["nz"] = nv[:, 0], nv[:, 1], nv[:, 2]
    pts["max_distance"] = dist * sf[k["octave"][idx]] * rng.uniform(0.9, 1.1, m)
    pts["min_distance"] = pts["max_distance"] / sf[7] * 0.8
    obs = rng.integers(0, 4, m).astype(np.int32)
    wp = np.zeros(m, pkg.WORLDPOINT_DTYPE)
    for f in ("valid", "wx", "wy", "wz", "nx", "ny", "nz", "max_distance", "min_distance"):
        wp[f] = pts[f]
    wp["observations"] = obs
    pd = d[idx] ^ _flips(rng, (m, 32))
    T = np.eye(4, dtype=np.float32)
    uright = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 30, n), -1).astype(np.float32)
    fm, ext = _presets(rng, n, m)
    proj = oracle.is_in_frustum(pts, obs, T, cam, oracle.grid_geom(W, H), 0.5, log_sf, 8)
    assert proj["in_view"].sum() > 0.5 * m
    on, ofm = oracle.search_by_projection_mp(k, d, uright, oracle.grid_geom(W, H), sf, proj, pd, fm, ext, 3.0, 0.8)
    thr = pkg.predict_scale_thresholds(log_sf, 8)
    gn, gfm, gproj = pkg.search_local_points(k, d, uright, pkg.grid_geom(W, H), sf, wp, pd, T, pcam, 0.5, thr, fm, ext, 3.0, 0.8)
    assert _path(pkg) == (pkg.RES_EXACT, pkg.FB_N, 0)
    assert on > 300 and gn == on
    np.testing.assert_array_equal(gfm, ofm)
    for f in proj.dtype.names:
        np.testing.assert_array_equal(gproj[f], proj[f], err_msg=f)


def test_single_wave_lds_past_48k(pkg, oracle, frame):
    """n > 24576 with m > 4096: the single-wave resolvers' dynamic LDS passes 48 KB (launched without hipFuncSetAttribute)."""
    for mode in (MODE_MP, MODE_FRAME):
        path, on = RUN[mode](pkg, oracle, frame, 25000, 4200, 600 + mode)
        assert on > 300
        assert _expect(pkg, mode, 4200, 25000, path) == pkg.RES_WAVE and path[2] > 48 * 1024


def test_keypoints_65535_65536(pkg, oracle, frame):
    """n = 65535 runs (exact kernel, oracle's result); 65536 is an argument error of every guided search, not a crash."""
    path, on = run_mp(pkg, oracle, frame, 65535, 1500, 700)
    assert path == (pkg.RES_EXACT, pkg.FB_N, 0) and on > 200
    rng = np.random.default_rng(701)
    k, d = _kps(frame, 65536, rng)
    mps, md = _mappoints(k, d, rng, 100)
    ur = np.full(65536, -1, np.float32)
    fm = np.full(65536, -1, np.int32)
    with pytest.raises(pkg.OrbxError) as e:
        pkg.ORBmatcher(0.8, True).SearchByProjection(k, d, ur, pkg.grid_geom(W, H), frame[2], mps, md, fm, None, 3.0)
    assert e.value.status == pkg.ORBX_ERR_ARG
    q = np.zeros(10, pkg.WINDOW_DTYPE)
    with pytest.raises(pkg.OrbxError) as e:
        pkg.match_windows(k, d, None, pkg.grid_geom(W, H), q, md[:10], fm, None, 100, True)
    assert e.value.status == pkg.ORBX_ERR_ARG
    k1 = k[:50].copy()
    with pytest.raises(pkg.OrbxError) as e:
        pkg.ORBmatcher(0.9, True).SearchForInitialization(k1, d[:50], k, d, pkg.grid_geom(W, H),
                                                          np.stack([k1["x"], k1["y"]], 1), 100)
    assert e.value.status == pkg.ORBX_ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------------------
# candidate lists: CAND_CAP and the QK kept candidates

def _outside(k, d, cx, cy, half):
    """k, d without the keypoints of the square of half-width `half` around (cx, cy)."""
    keep = (np.abs(k["x"] - cx) >= half) | (np.abs(k["y"] - cy) >= half)
    return k[keep], d[keep]


@pytest.mark.parametrize("count", [CAND_CAP, CAND_CAP + 1])
def test_cand_cap_windows(pkg, oracle, frame, count):
    """k_cand<false>: one query whose window holds exactly 512, then 513 eligible keypoints (513: the fast path reports the overflow
    and the exact kernel runs), among the frame's ordinary keypoints and queries."""
    rng = np.random.default_rng(800 + count)
    k0, d0 = _outside(*_kps(frame, 2100, rng), 900.0, 500.0, 12.0)
    k0, d0 = k0[:2000], d0[:2000]
    kc, dc = _cluster(frame, count, rng)
    k, d = np.concatenate([k0, kc]), np.concatenate([d0, dc])
    n = len(k)
    m = 300
    q = np.zeros(m, pkg.WINDOW_DTYPE)
    qi = rng.choice(2000, m, replace=False)
    q["valid"] = 1
    q["u"], q["v"] = k0["x"][qi] + rng.normal(0, 1, m), k0["y"][qi] + rng.normal(0, 1, m)
    q["radius"] = 4.0
    q["min_level"], q["max_level"] = -1, 8
    q["angle"] = k0["angle"][qi]
    q["blocks"] = 1
    q["ur_tol"] = -1
    q[0] = (1, 900.0, 500.0, 7.0, -1, 8, 0.0, 1, 0.0, -1.0)
    qd = d0[qi] ^ _flips(rng, (m, 32), 3)
    qd[0] = dc[0] ^ _flips(rng, 32, 2)
    holder = np.full(n, -1, np.int32)
    L = pkg.matcher_lib()
    L.orbm_set_thread_option(2, 1)
    en, eh = pkg.match_windows(k, d, None, pkg.grid_geom(W, H), q, qd, holder, None, 100, True)
    assert _path(pkg) == (pkg.RES_EXACT, pkg.FB_OPTION, 0)
    L.orbm_set_thread_option(2, 0)
    gn, gh = pkg.match_windows(k, d, None, pkg.grid_geom(W, H), q, qd, holder, None, 100, True)
    assert gn == en > 50
    np.testing.assert_array_equal(gh, eh)
    ck = pkg.debug_features_in_area(k, pkg.grid_geom(W, H), 900.0, 500.0, 7.0)
    assert len(ck) == count
    if count <= CAND_CAP:
        _expect(pkg, MODE_WIN, m, n, _path(pkg))
    else:
        assert _path(pkg)[:2] == (pkg.RES_EXACT, pkg.FB_CAND_CAP)


@pytest.mark.parametrize("count", [CAND_CAP, CAND_CAP + 1])
def test_cand_cap_initialization(pkg, oracle, frame, count):
    """k_cand<true> (SearchForInitialization keeps the whole sorted list): one F1 keypoint whose window holds 512 / 513 F2
    keypoints."""
    k1, d1, k2, d2, prev = cand_cap_init_inputs(frame, count)
    on, om12, oprev = oracle.search_for_initialization(k1, d1, k2, d2, oracle.grid_geom(W, H), prev, 10, 0.9, True)
    gn, gm12, gprev = pkg.ORBmatcher(0.9, True).SearchForInitialization(k1, d1, k2, d2, pkg.grid_geom(W, H), prev, 10)
    assert gn == on
    np.testing.assert_array_equal(gm12, om12)
    np.testing.assert_array_equal(gprev, oprev)
    if count <= CAND_CAP:
        _expect(pkg, MODE_INIT, 400, count, _path(pkg))
    else:
        assert _path(pkg)[:2] == (pkg.RES_EXACT, pkg.FB_CAND_CAP)


def test_ties_past_the_kept_candidates(pkg, oracle, frame):
    """More than QK = 8 candidates at the same best Hamming distance, and blocking that forces the resolver past the kept eight: the
    fast path notices (a query ran out of its candidates) and the exact kernel's result is the oracle's."""
    rng = np.random.default_rng(900)
    k0, d0 = _outside(*_kps(frame, 1500, rng), 700.0, 300.0, 10.0)
    kc, _ = _cluster(frame, 12, rng, cx=700.0, cy=300.0, half=3.0)
    dc = np.repeat(d0[:1], 12, axis=0)                     # twelve keypoints, one descriptor: equal distance to every query
    k, d = np.concatenate([k0, kc]), np.concatenate([d0, dc])
    n = len(k)
    m = 40
    q = np.zeros(m, pkg.WINDOW_DTYPE)
    q["valid"] = 1
    q["u"], q["v"], q["radius"] = 700.0, 300.0, 5.0
    q["min_level"], q["max_level"] = -1, 8
    q["blocks"] = 1
    q["ur_tol"] = -1
    qd = np.repeat(d0[:1], m, axis=0) ^ _flips(rng, (m, 32), 5)
    holder = np.full(n, -1, np.int32)
    L = pkg.matcher_lib()
    L.orbm_set_thread_option(2, 1)
    en, eh = pkg.match_windows(k, d, None, pkg.grid_geom(W, H), q, qd, holder, None, 256, False)
    L.orbm_set_thread_option(2, 0)
    gn, gh = pkg.match_windows(k, d, None, pkg.grid_geom(W, H), q, qd, holder, None, 256, False)
    assert _path(pkg)[:2] == (pkg.RES_EXACT, pkg.FB_QK)
    assert gn == en >= 12
    np.testing.assert_array_equal(gh, eh)
    # the same through SearchByProjection(F, MPs) against the oracle: observations > 0 block, equal distances everywhere
    mps = np.zeros(m, [("in_view", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("level", "<i4"),
                       ("view_cos", "<f4"), ("observations", "<i4")])
    mps["in_view"], mps["proj_x"], mps["proj_y"], mps["proj_xr"] = 1, 700.0, 300.0, 690.0
    mps["level"], mps["view_cos"], mps["observations"] = 0, 1.0, 1
    k[n - 12:]["octave"] = 0
    path, on = run_mp(pkg, oracle, frame, n, m, 901, th=1.5, ratio=1.0, kd=(k, d), mps=(mps, qd), presets=False)
    assert path[:2] == (pkg.RES_EXACT, pkg.FB_QK) and on >= 12


def test_ratio_test_ties(pkg, oracle, frame):
    """best == second (equal distance, same level): the ratio test rejects; the fast resolvers agree with the oracle."""
    rng = np.random.default_rng(950)
    k, d = _kps(frame, 3000, rng)
    pairs = rng.choice(2900, 400, replace=False)
    d[pairs + 1] = d[pairs]                                 # a twin with the same descriptor beside each of 400 keypoints
    k["x"][pairs + 1] = k["x"][pairs] + 0.5
    k["y"][pairs + 1] = k["y"][pairs]
    k["octave"][pairs + 1] = k["octave"][pairs]
    mps = np.zeros(1500, [("in_view", "<i4"), ("proj_x", "<f4"), ("proj_y", "<f4"), ("proj_xr", "<f4"), ("level", "<i4"),
                          ("view_cos", "<f4"), ("observations", "<i4")])
    sel = np.concatenate([pairs, rng.choice(3000, 1100, replace=False)])
    mps["in_view"] = 1
    mps["proj_x"], mps["proj_y"] = k["x"][sel] + 0.25, k["y"][sel]
    mps["proj_xr"] = mps["proj_x"] - 10
    mps["level"] = k["octave"][sel]
    mps["view_cos"] = 1.0
    mps["observations"] = rng.integers(0, 2, 1500)
    md = d[sel] ^ _flips(rng, (1500, 32))
    for ratio in (0.8, 1.0):
        path, on = run_mp(pkg, oracle, frame, 3000, 1500, 951, th=1.0, ratio=ratio, kd=(k, d), mps=(mps, md))
        assert path[0] in (pkg.RES_PAR_Q2, pkg.RES_EXACT) and on > 300


# ---------------------------------------------------------------------------------------------------------------------------------
# SearchForInitialization: n2 = 7000 / 7001

def _init_case(pkg, oracle, frame, n1, n2, seed, window=30, contention=False):
    k1, d1, k2, d2, prev = init_inputs(frame, n1, n2, seed, contention)
    on, om12, oprev = oracle.search_for_initialization(k1, d1, k2, d2, oracle.grid_geom(W, H), prev, window, 0.9, True)
    gn, gm12, gprev = pkg.ORBmatcher(0.9, True).SearchForInitialization(k1, d1, k2, d2, pkg.grid_geom(W, H), prev, window)
    assert gn == on, (gn, on, _path(pkg))
    np.testing.assert_array_equal(gm12, om12)
    np.testing.assert_array_equal(gprev, oprev)
    return _path(pkg), on


def test_initialization_7000_7001(pkg, oracle, frame):
    path, on = _init_case(pkg, oracle, frame, 3000, 7000, 1000)
    assert on > 300
    _expect(pkg, MODE_INIT, 3000, 7000, path)
    path, on = _init_case(pkg, oracle, frame, 3000, 7001, 1001)
    assert path == (pkg.RES_EXACT, pkg.FB_INIT_SIZE, 0) and on > 300
    path, on = _init_case(pkg, oracle, frame, 3000, 7000, 1002, window=100, contention=True)
    assert on > 10 and path[0] in (pkg.RES_WAVE, pkg.RES_EXACT)


# ---------------------------------------------------------------------------------------------------------------------------------
# sizes that change from call to call on one host thread (the arena grows and is reused, the pinned mirror with it)

def test_sizes_change_between_calls(pkg, oracle, frame):
    lo = int(_old_rule_windows(pkg, MODE_MP, 2000)[0]) if len(_old_rule_windows(pkg, MODE_MP, 2000)) else 11830
    seq = [(1200, 800), (lo, 2000), (30001, 2000), (1200, 800), (4097, 3000), (900, 4500), (1200, 800)]
    for i, (n, m) in enumerate(seq):
        path, on = run_mp(pkg, oracle, frame, n, m, 1100 + i)
        assert on > 100
        if n <= 30000:
            _expect(pkg, MODE_MP, m, n, path)
        else:
            assert path == (pkg.RES_EXACT, pkg.FB_N, 0)
    for i, (n, m) in enumerate([(1200, 800), (lo, 2000), (1200, 800)]):
        path, on = run_frame(pkg, oracle, frame, n, m, 1200 + i)
        _expect(pkg, MODE_FRAME, m, n, path)


# ---------------------------------------------------------------------------------------------------------------------------------
# the three resolver options at one size of each group

@pytest.mark.parametrize("option", ["fast", "fast_wave", "exact"])
def test_resolver_options_agree(pkg, oracle, frame, option):
    L = pkg.matcher_lib()
    L.orbm_set_thread_option(2, 1 if option == "exact" else 0)
    L.orbm_set_thread_option(3, 1 if option == "fast_wave" else 0)
    for mode, n, m in ((MODE_MP, 2049, 2049), (MODE_FRAME, 4097, 3000), (MODE_WIN, 11840, 2000), (MODE_MP, 30000, 1500)):
        path, on = RUN[mode](pkg, oracle, frame, n, m, 1300 + n + mode)
        assert on > 200
        if option == "exact":
            assert path == (pkg.RES_EXACT, pkg.FB_OPTION, 0)
        elif option == "fast_wave":
            assert path[:2] == (pkg.RES_WAVE, pkg.FB_NONE)
        else:
            _expect(pkg, mode, m, n, path)
    path, on = _init_case(pkg, oracle, frame, 2000, 7000, 1399)
    assert path[0] == (pkg.RES_EXACT if option == "exact" else pkg.RES_WAVE)


# ---------------------------------------------------------------------------------------------------------------------------------
# stereo matcher (Frame::ComputeStereoMatches, src/Frame.cc:481-655)

UW, UH = 3840, 2160
S_MBF, S_FX = 47.9, 435.2


@pytest.fixture(scope="module")
def uhd(oracle, synth):
    """A 3840x2160 pair and its oracle extraction with 8000 features (replicated past SM_LDS_CAP keypoints per image below)."""
    left, right = synth.stereo_pair_blocky(UW, UH, 61)
    nf = 8000
    orl, orr = oracle.Extractor(nf, 1.2, 8, 20, 7), oracle.Extractor(nf, 1.2, 8, 20, 7)
    kl, dl = orl.extract(left)
    kr, dr = orr.extract(right)
    pl = [orl.pyramid_level(i) for i in range(8)]
    pr = [orr.pyramid_level(i) for i in range(8)]
    return dict(left=left, right=right, nf=nf, kl=kl, dl=dl, kr=kr, dr=dr, pl=pl, pr=pr, sf=orl.scale_factors,
                isf=orl.inv_scale_factors)


def _bins(rows, sf_last, span=6, max_bins=512):
    band = int(np.float32(4.0) * np.float32(sf_last)) + 4
    s = 0
    while ((band - 1) >> s) + 2 > span:
        s += 1
    while (rows + (1 << s) - 1) >> s > max_bins:
        s += 1
    return s, max(1, (rows + (1 << s) - 1) >> s)


def _stereo(pkg, oracle, u, exl, exr, kl, dl, kr, dr):
    mb = float(np.float32(S_MBF) / np.float32(S_FX))
    ur, dp, n = pkg.compute_stereo_matches(exl, exr, kl, dl, kr, dr, S_MBF, mb)
    on, our, odp = oracle.stereo_match(kl, dl, kr, dr, u["pl"], u["pr"], u["sf"], u["isf"], S_MBF, mb)
    assert n == on
    np.testing.assert_array_equal(ur, our)
    np.testing.assert_array_equal(dp, odp)
    return pkg.debug_stereo_path(), on


@pytest.fixture(scope="module")
def uhd_ex(pkg, uhd):
    old = pkg.default_developer
    pkg.default_developer = True
    exl, exr = pkg.ORBextractor(uhd["nf"], 1.2, 8, 20, 7), pkg.ORBextractor(uhd["nf"], 1.2, 8, 20, 7)
    pkg.default_developer = old
    kl, dl = exl(uhd["left"])
    kr, dr = exr(uhd["right"])
    np.testing.assert_array_equal(dl, uhd["dl"])
    np.testing.assert_array_equal(dr, uhd["dr"])
    return exl, exr


@pytest.mark.parametrize("nl,nr", [(12288, 12288), (12289, 6000), (6000, 12289)])
def test_stereo_sm_lds_cap(pkg, oracle, uhd, uhd_ex, nl, nr):
    """nl or nr = 12288 / 12289 (SM_LDS_CAP: the SAD median leaves LDS for global memory), on 3840x2160 (bhShift 3)."""
    u = uhd
    il, ir = np.arange(nl) % len(u["kl"]), np.arange(nr) % len(u["kr"])
    path, on = _stereo(pkg, oracle, u, *uhd_ex, u["kl"][il], u["dl"][il], u["kr"][ir], u["dr"][ir])
    assert on > 500
    assert path[:3] == ((1 if max(nl, nr) <= 12288 else 0),) + _bins(UH, u["sf"][7])
    assert path[1] == 3


def test_stereo_candidate_list_restarts(pkg, oracle, uhd, uhd_ex):
    """More than ST_CAND = 256 candidate right keypoints in one left keypoint's band: the list is scored and restarted.  The right
    keypoints are copies, interleaved, so equal Hamming distances and equal SAD values sit on both sides of the 256 boundary and the
    first minimum in iR order must win."""
    u = uhd
    kl, dl, kr, dr = u["kl"], u["dl"], u["kr"], u["dr"]
    for y0 in range(200, 2000, 7):   # a row with a left keypoint (octave <= 1) that has a right keypoint of octave 0 in its u range
        band = np.flatnonzero((kr["octave"] == 0) & (np.abs(kr["y"] - y0) < 1))
        left = np.flatnonzero((kl["octave"] <= 1) & (np.abs(kl["y"] - y0) < 1))
        du = kl["x"][left][:, None] - kr["x"][band][None, :]
        if len(band) and len(left) and ((du >= 1) & (du <= 400)).any():
            break
    else:
        pytest.fail("no row with a left / right pair")
    ir = np.concatenate([np.tile(band, 300), np.arange(len(kr))])   # every band entry 300 times, interleaved
    il = np.concatenate([left, np.arange(min(len(kl), 3000))])
    path, on = _stereo(pkg, oracle, u, *uhd_ex, kl[il], dl[il], kr[ir], dr[ir])
    assert path[3] == 1 and on > 100
    path, on = _stereo(pkg, oracle, u, *uhd_ex, kl[:3000], dl[:3000], kr[:3000], dr[:3000])
    assert path[3] == 0


def test_stereo_frame_capacity_past_lds_cap(pkg, oracle, synth, hooks):
    """stereo_frame / stereo_frame_view with an extractor whose per-image capacity exceeds 12288: k_stereo_finish without LDS, over
    several workgroups (13000 features over 16 levels of scale 1.1: the quad-tree's LDS plan takes that many at 1920x1080)."""
    w, h, nf, sf, nl = 1920, 1080, 13000, 1.1, 16
    left, right = synth.stereo_pair_blocky(w, h, 81)
    orl, orr = oracle.Extractor(nf, sf, nl, 20, 7), oracle.Extractor(nf, sf, nl, 20, 7)
    kl, dl = orl.extract(left)
    kr, dr = orr.extract(right)
    ex = pkg.ORBextractor(nf, sf, nl, 20, 7)
    assert ex.max_keypoints() > 12288
    mb = float(np.float32(S_MBF) / np.float32(S_FX))
    on, our, odp = oracle.stereo_match(kl, dl, kr, dr, [orl.pyramid_level(i) for i in range(nl)],
                                       [orr.pyramid_level(i) for i in range(nl)], orl.scale_factors, orl.inv_scale_factors, S_MBF, mb)
    assert on > 500
    for view in (False, True, True):
        r = ex.stereo_frame_view(left, right, S_MBF, mb) if view else ex.stereo_frame(left, right, S_MBF, mb)
        np.testing.assert_array_equal(r["dl"], dl)
        np.testing.assert_array_equal(r["dr"], dr)
        assert r["nmatch"] == on
        np.testing.assert_array_equal(r["uright"], our)
        np.testing.assert_array_equal(r["depth"], odp)
        assert pkg.debug_stereo_path()[:3] == (0,) + _bins(h, orl.scale_factors[nl - 1])


@pytest.mark.parametrize("sf,nl", [(1.5, 8), (2.6, 3)])
def test_stereo_bin_geometry(pkg, oracle, synth, hooks, sf, nl):
    """Scale factors / level counts whose coarsest band forces wider bins."""
    w, h = 1920, 1080
    left, right = synth.stereo_pair_blocky(w, h, 71)
    orl, orr = oracle.Extractor(2000, sf, nl, 20, 7), oracle.Extractor(2000, sf, nl, 20, 7)
    kl, dl = orl.extract(left)
    kr, dr = orr.extract(right)
    exl, exr = pkg.ORBextractor(2000, sf, nl, 20, 7), pkg.ORBextractor(2000, sf, nl, 20, 7)
    gkl, gdl = exl(left)
    gkr, gdr = exr(right)
    np.testing.assert_array_equal(gdl, dl)
    np.testing.assert_array_equal(gdr, dr)
    u = dict(pl=[orl.pyramid_level(i) for i in range(nl)], pr=[orr.pyramid_level(i) for i in range(nl)], sf=orl.scale_factors,
             isf=orl.inv_scale_factors)
    path, on = _stereo(pkg, oracle, u, exl, exr, kl, dl, kr, dr)
    assert on > 50
    assert path[1:3] == _bins(h, orl.scale_factors[nl - 1])
    assert path[1] > _bins(h, np.float32(1.2) ** 7)[0]


def test_stereo_cap_over_65535_is_an_error(pkg, uhd, uhd_ex):
    u = uhd
    il = np.arange(65536) % len(u["kl"])
    with pytest.raises(pkg.OrbxError) as e:
        pkg.compute_stereo_matches(*uhd_ex, u["kl"][il], u["dl"][il], u["kr"][:100], u["dr"][:100], S_MBF, 0.11)
    assert e.value.status == pkg.ORBX_ERR_UNSUPPORTED
