"""Scenes of the matcher tests that more than one file runs: the builders of tests/test_match_gpu.py and
tests/test_match_limits_gpu.py (moved here unchanged), and on top of them the fixed list of matcher calls with their
oracle results that tests/match_threads_worker.py replays from several host threads at once.

Nothing here touches the GPU: a builder returns host arrays, a Case holds its expected result (computed once by the CPU
oracle, never modified) and a function that makes the library call when a thread asks for it."""
import numpy as np

import bow_scene as bs
import kf_scene as ks


# ---- builders of tests/test_match_gpu.py --------------------------------------------------------------------------
def features(oracle, img, nf=1000):
    orc = oracle.Extractor(nf, 1.2, 8, 20, 7)
    k, d = orc.extract(img)
    return orc, k, d


def mappoints_from(oracle, k, d, rng, m):
    idx = rng.choice(len(k), size=m, replace=len(k) < m)
    mps = np.zeros(m, oracle.MP_DTYPE)
    mps["in_view"] = rng.random(m) > 0.1
    mps["proj_x"] = k["x"][idx] + rng.normal(0, 1.5, m)
    mps["proj_y"] = k["y"][idx] + rng.normal(0, 1.5, m)
    mps["proj_xr"] = mps["proj_x"] - rng.uniform(1, 30, m)
    mps["level"] = np.clip(k["octave"][idx] + rng.integers(-1, 2, m), 0, 7)
    mps["view_cos"] = rng.uniform(0.99, 1.0, m)
    mps["observations"] = rng.integers(0, 4, m)
    md = d[idx].copy()
    flip = rng.integers(0, 256, md.shape, dtype=np.uint8) & rng.integers(0, 256, md.shape, dtype=np.uint8) & \
        rng.integers(0, 256, md.shape, dtype=np.uint8) & rng.integers(0, 256, md.shape, dtype=np.uint8)
    return mps, md ^ flip


def kfside(oracle, synth, seed, distorted, m=1800, w=1241, h=376):
    rng = np.random.default_rng(seed)
    _, k, d = features(oracle, synth.frame(w, h, 30 + seed), 1000)
    sf = oracle.Extractor(1000, 1.2, 8, 20, 7).scale_factors
    cam = oracle.Cam(ks.FX, ks.FY, ks.CX, ks.CY, ks.MBF, np.float32(ks.MBF) / np.float32(ks.FX))
    return ks, w, h, rng, k, d, sf, cam, np.float32(np.log(np.float32(1.2))), m


def local_map(pkg, oracle, synth, seed, m=3000):
    ks_, w, h, rng, k, d, sf, cam, log_sf, _ = kfside(oracle, synth, seed, False, m)
    T = ks.pose(rng)
    pts3, pd, idx = ks.points_for(oracle, rng, k, d, sf, T, m, bits=3)
    pts3["valid"] = rng.random(m) > 0.1
    # level boundaries: make max_distance/dist land within a few ulps of sf^k for part of the points
    R, t = T[:3, :3].astype(np.float64), T[:3, 3].astype(np.float64)
    Ow = (-R.T @ t).astype(np.float32)
    dist = np.sqrt(((np.stack([pts3["wx"], pts3["wy"], pts3["wz"]], 1) - Ow).astype(np.float64) ** 2).sum(1)).astype(np.float32)
    edge = rng.random(m) < 0.3
    kk = rng.integers(0, 8, m)
    ulp = rng.integers(-3, 4, m)
    target = (np.float32(1.2) ** kk).astype(np.float32)
    md = (dist * target).astype(np.float32)
    md = (md.view(np.int32) + ulp.astype(np.int32)).view(np.float32)
    pts3["max_distance"] = np.where(edge, md, pts3["max_distance"])
    pts3["min_distance"] = np.where(edge, md * np.float32(0.1), pts3["min_distance"])
    obs = rng.integers(0, 6, m).astype(np.int32)
    wp = np.zeros(m, pkg.WORLDPOINT_DTYPE)
    for f in ("valid", "wx", "wy", "wz", "nx", "ny", "nz", "max_distance", "min_distance"):
        wp[f] = pts3[f]
    wp["observations"] = obs
    return ks, w, h, rng, k, d, sf, cam, log_sf, T, pts3, wp, pd, obs


# ---- builders of tests/test_match_limits_gpu.py ---------------------------------------------------------------------
W, H = 1920, 1080


def limits_frame(oracle, synth):
    """One 1920x1080 / 4000-feature extraction (the oracle's: bit-identical to the HIP extractor, tested elsewhere)."""
    orc = oracle.Extractor(4000, 1.2, 8, 20, 7)
    k, d = orc.extract(synth.frame(W, H, 51))
    assert len(k) > 3000
    return k, d, orc.scale_factors


def flips(rng, shape, ands=4):
    f = rng.integers(0, 256, shape, dtype=np.uint8)
    for _ in range(ands - 1):
        f &= rng.integers(0, 256, shape, dtype=np.uint8)
    return f


def kps(frame, n, rng):
    """n keypoints: the extracted ones first, then jittered replicas (descriptors with sparse bit flips); the jitter stays inside the
    extracted keypoints' bounding box, which lies inside every level's border margin."""
    k, d, _ = frame
    idx = np.arange(n) % len(k)
    kk, dd = k[idx].copy(), d[idx].copy()
    rep = np.arange(n) >= len(k)
    r = int(rep.sum())
    if r:
        kk["x"][rep] = np.clip(kk["x"][rep] + rng.normal(0, 1.0, r), k["x"].min(), k["x"].max()).astype(np.float32)
        kk["y"][rep] = np.clip(kk["y"][rep] + rng.normal(0, 1.0, r), k["y"].min(), k["y"].max()).astype(np.float32)
        dd[rep] ^= flips(rng, (r, 32))
    return kk, dd


def cluster(frame, count, rng, cx=900.0, cy=500.0, half=6.0):
    """count keypoints of octave 0 inside a square of half-width `half` around (cx, cy): one query window holds all of them."""
    k, d, _ = frame
    src = np.flatnonzero(k["octave"] == 0)
    idx = src[np.arange(count) % len(src)]
    kk, dd = k[idx].copy(), d[idx].copy()
    kk["x"] = (cx + rng.uniform(-half, half, count)).astype(np.float32)
    kk["y"] = (cy + rng.uniform(-half, half, count)).astype(np.float32)
    dd ^= flips(rng, (count, 32), 2)
    return kk, dd


def init_inputs(frame, n1, n2, seed, contention=False):
    """SearchForInitialization on replicated keypoints of the 1920x1080 frame -> (k1, d1, k2, d2, prev)."""
    rng = np.random.default_rng(seed)
    k2, d2 = kps(frame, n2, rng)
    if contention:   # every F1 keypoint fights for the same few F2 keypoints
        src = rng.choice(60, n1)
        k1, d1 = k2[src].copy(), d2[src] ^ flips(rng, (n1, 32), 3)
    else:
        k1, d1 = kps(frame, n1, rng)
    k1["octave"] = 0
    k2["octave"] = 0
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32) + rng.normal(0, 2, (n1, 2)).astype(np.float32)
    return k1, d1, k2, d2, prev


def cand_cap_init_inputs(frame, count):
    """One F1 keypoint whose window (10 px) holds `count` F2 keypoints -> (k1, d1, k2, d2, prev)."""
    rng = np.random.default_rng(850 + count)
    k2, d2 = cluster(frame, count, rng)
    k1, d1 = kps(frame, 400, rng)
    k1["octave"] = 0
    k1["x"][0], k1["y"][0] = 900.0, 500.0
    d1[0] = d2[5] ^ flips(rng, 32, 2)
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    return k1, d1, k2, d2, prev


# ---- the per-thread scratch: minimum capacities and what a call needs (restated from csrc/, see each line) -----------
ARENA_MIN, STAGE_MIN, BOW_MIN = 4 << 20, 1 << 20, 1 << 20      # arena_begin, stage_reserve, scratch: max(2 * need, this)
QK, CAND_CAP = 8, 512


def _aln(x):
    return (x + 255) & ~255


def arena_need_local_points(n, m):
    """fast_search_by_projection_mp (csrc/orbx_match_fast.hip): n keypoints, m world points (40-byte orbm_worldpoint_t)."""
    return n * (28 + 32 + 32 + 16) + m * (28 + 32 + QK * 8 + 64 + 40) + 65536


def stage_need_initialization(n1, n2):
    """orbm_search_for_initialization's exact kernel (csrc/orbx_match.hip): the StagePlan of its eleven arrays."""
    return (_aln(28 * n1) + _aln(32 * n1) + _aln(28 * n2) + _aln(32 * n2) + _aln(8 * n1) + _aln(4 * n1) + _aln(4) + _aln(4 * n2) + _aln(4 * n2) +
            _aln(2 * n2) + _aln(4 * n1))


def bow_need_triangulation(nq, nc, nnodes, tq, tc):
    """orbm_search_for_triangulation (csrc/orbx_bow.hip): the fourteen arrays it lays out in the BowScratch."""
    return (_aln(28 * nq) + _aln(32 * nq) + _aln(nq) + _aln(4 * nq) + _aln(28 * nc) + _aln(32 * nc) + _aln(nc) + _aln(4 * nc) +
            2 * _aln(4 * (nnodes + 1)) + _aln(4 * max(tq, 1)) + _aln(4 * max(tc, 1)) + _aln(4 * nq) + _aln(16))


# ---- the calls the threaded worker replays ----------------------------------------------------------------------------
class Case:
    """One library call with its expected result.  want: {field: ndarray or int}, from the CPU oracle; run(pkg, shared) makes the
    call and returns the same fields; guided: the call leaves a path record (orbm_debug_match_path)."""

    def __init__(self, name, run, want, guided=False):
        self.name, self.run, self.want, self.guided = name, run, want, guided


def gpu_bow(pkg, s, variant, ratio, ori):
    v = bs.VARIANTS[variant]
    return pkg.search_by_bow(s["qd"], s["qa"], s["qv"], s["cd"], s["ca"], s["cv"] if v["use_cv"] else None, s["nqs"], s["qit"], s["ncs"],
                             s["cit"], v["max_dist"], ratio, ori)


def gpu_tri(pkg, s, g, ori, max_dist=50):
    return pkg.search_for_triangulation(g["k1"], s["qd"], g["f1"], g["k2"], s["cd"], g["f2"], s["nqs"], s["qit"], s["ncs"], s["cit"],
                                        g["F12"], g["ex"], g["ey"], g["sf"], g["sigma2"], max_dist, ori)


def _tri_case(oracle, name, s, g):
    n, mq = bs.oracle_tri(oracle, s, g, True)
    assert n > 100, (name, n)
    return Case(name, lambda pkg, shared: dict(zip(("nmatches", "match_q"), gpu_tri(pkg, s, g, True))), {"nmatches": n, "match_q": mq})


def triangulation_capacity():
    """The BowScratch's capacity once the crowded case has run: max(2 * need, 1 MiB) (scratch, csrc/orbx_bow.hip)."""
    nq, nc = sum(bs.CROWD_Q), sum(bs.CROWD_C)
    return max(BOW_MIN, 2 * bow_need_triangulation(nq, nc, len(bs.CROWD_Q), nq, nc))


def big_triangulation_sizes():
    """The crowded node sizes plus two full nodes and the smallest further node with which orbm_search_for_triangulation needs more
    than the BowScratch holds after the crowded case."""
    for extra in range(0, 4097, 8):
        sq, sc = bs.CROWD_Q + (150, 100, 60), bs.CROWD_C + (4096, 4096, extra)
        if bow_need_triangulation(sum(sq), sum(sc), len(sq), sum(sq), sum(sc)) > triangulation_capacity():
            return sq, sc
    raise AssertionError("no size found")


def local_mapping_cases(pkg, oracle, synth):
    """LocalMapping's calls: SearchForTriangulation at the crowded nodes, and the device part of Fuse (orbm_best_in_windows with the
    reprojection gate, orbm_match_windows) on a 640x480 / 1000-feature frame with 1500 queries.  -> (cases, the BowScratch regrow)"""
    s, g = bs.tri_case()
    cases = [_tri_case(oracle, "search_for_triangulation", s, g)]
    _, w, h, rng, k, d, sf, cam, log_sf, m = kfside(oracle, synth, 8, False, 1500, 640, 480)
    T = ks.pose(rng)
    pts, pd, _ = ks.points_for(oracle, rng, k, d, sf, T, m)
    og, oga, _ = ks.geoms(oracle, w, h, False)
    pg, pga, _ = ks.geoms(pkg, w, h, False)
    q = oracle.pose_window_queries(pts, og, sf, log_sf, cam, T, 3.0)
    uright = np.where(rng.random(len(k)) < 0.5, k["x"] - rng.uniform(1, 40, len(k)), -1).astype(np.float32)
    inv_s2 = (1.0 / (sf * sf)).astype(np.float32)
    obi, obd = oracle.best_in_windows(k, d, uright, og, q, pd, inv_s2, oga)
    assert (obi >= 0).sum() > 300
    cases.append(Case("best_in_windows", lambda pkg, shared: dict(zip(("best_idx", "best_dist"), pkg.best_in_windows(k, d, uright, pg, q, pd, inv_s2, 0, pga))),
                      {"best_idx": obi, "best_dist": obd}))
    S = ks.pose(rng, scale=1.07)
    pts2, pd2, _ = ks.points_for(oracle, rng, k, d, sf, S, m, scale=1.07)
    pts2["valid"] = rng.random(m) > 0.1
    matched = np.full(len(k), -1, np.int32)
    matched[rng.choice(len(k), 60, replace=False)] = -2
    on, om = oracle.search_by_projection_sim3(k, d, og, sf, log_sf, cam, S, pts2, pd2, matched, 10, oga)
    q2 = oracle.sim3_window_queries(pts2, og, sf, log_sf, cam, S, 10.0)
    assert on > 200
    cases.append(Case("match_windows", lambda pkg, shared: dict(zip(("nmatches", "holder"), pkg.match_windows(k, d, None, pg, q2, pd2, matched, None, 50, False, 0, pga))),
                      {"nmatches": on, "holder": om}, guided=True))
    sq, sc = big_triangulation_sizes()
    sb = bs.crowded_nodes(sq, sc, 14, twins=0.5)
    big = _tri_case(oracle, "search_for_triangulation_big", sb, bs.tri_geometry(sb, 15))
    big.need, big.before = bow_need_triangulation(len(sb["qa"]), len(sb["ca"]), len(sq), sum(sq), sum(sc)), triangulation_capacity()
    return cases, big


def loop_closing_cases(pkg, oracle, synth, frame):
    """LoopClosing's calls: SearchByBoW (both variants) at the crowded nodes, the vocabulary descent, SearchByProjection(F, MPs)
    with 1500 map points, SearchForInitialization on the fast path (640x480, 1000 features) and with a window of 513 candidates (the
    exact kernel: the staging pair).  -> (cases, the staging pair's regrow); shared["voc"] is the device vocabulary."""
    s = bs.crowded_case()
    cases = []
    for variant in ("kf_frame", "kf_kf"):
        n, mq = bs.oracle_bow(oracle, s, variant, 0.9, True)
        assert n > 100
        cases.append(Case("search_by_bow_" + variant, lambda pkg, shared, v=variant: dict(zip(("nmatches", "match_q"), gpu_bow(pkg, s, v, 0.9, True))),
                          {"nmatches": n, "match_q": mq}))
    voc = vocabulary()
    feats = bs.features_near_words(np.random.default_rng(42), voc, 1000)
    ov = oracle.Vocabulary(10, 3, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    want = [ov.transform_one(f, 1) for f in feats]
    cases.append(Case("orbv_transform", lambda pkg, shared: dict(zip(("word", "node", "weight"), shared["voc"].transform(feats, 1))),
                      {"word": np.array([x[0] for x in want], np.int32), "node": np.array([x[2] for x in want], np.int32),
                       "weight": np.array([x[1] for x in want], np.float64)}))
    w, h = 1241, 376
    _, k, d = features(oracle, synth.frame(w, h, 11), 1000)
    rng = np.random.default_rng(9)
    sf = oracle.Extractor(1000, 1.2, 8, 20, 7).scale_factors
    mps, md = mappoints_from(oracle, k, d, rng, 1500)
    uright = np.where(rng.random(len(k)) < 0.5, k["x"] - rng.uniform(1, 30, len(k)), -1).astype(np.float32)
    frame_mp = np.full(len(k), -1, np.int32)
    ext = np.zeros(len(k), np.int32)
    pre = rng.choice(len(k), 50, replace=False)
    frame_mp[pre] = -2
    ext[pre] = rng.integers(0, 2, 50)
    on, ofm = oracle.search_by_projection_mp(k, d, uright, oracle.grid_geom(w, h), sf, mps, md, frame_mp, ext, 3.0, 0.8)
    assert on > 100
    cases.append(Case("search_by_projection", lambda pkg, shared: dict(zip(("nmatches", "frame_mp"), pkg.ORBmatcher(0.8, True).SearchByProjection(
        k, d, uright, pkg.grid_geom(w, h), sf, mps, md, frame_mp, ext, 3.0))), {"nmatches": on, "frame_mp": ofm}, guided=True))
    img1 = synth.frame(640, 480, 7)
    img2 = np.roll(img1, (3, 5), axis=(0, 1))
    img2 = np.clip(img2.astype(np.int16) + np.random.default_rng(5).integers(-3, 4, img2.shape), 0, 255).astype(np.uint8)
    _, k1, d1 = features(oracle, img1, 1000)
    _, k2, d2 = features(oracle, img2, 1000)
    prev = np.stack([k1["x"], k1["y"]], 1).astype(np.float32)
    cases.append(_init_case(pkg, oracle, "search_for_initialization", (k1, d1, k2, d2, prev), 640, 480, 100, 30))
    cases.append(_init_case(pkg, oracle, "search_for_initialization_513", init_513_inputs(frame), W, H, 10, 100))
    n1 = 7001
    while stage_need_initialization(n1, 7001) <= STAGE_MIN:     # n2 = 7001: past k_resolve_init's LDS plan, the exact kernel runs
        n1 += 1
    big = _init_case(pkg, oracle, "search_for_initialization_big", init_inputs(frame, n1, 7001, 1001), W, H, 30, 300)
    big.need, big.before = stage_need_initialization(n1, 7001), STAGE_MIN
    return cases, big


def _init_case(pkg, oracle, name, inputs, w, h, window, at_least):
    k1, d1, k2, d2, prev = inputs
    on, om12, oprev = oracle.search_for_initialization(k1, d1, k2, d2, oracle.grid_geom(w, h), prev, window, 0.9, True)
    assert on > at_least, (name, on)

    def run(pkg, shared):
        return dict(zip(("nmatches", "matches12", "prev_matched"), pkg.ORBmatcher(0.9, True).SearchForInitialization(k1, d1, k2, d2, pkg.grid_geom(w, h), prev, window)))
    return Case(name, run, {"nmatches": on, "matches12": om12, "prev_matched": oprev}, guided=True)


def init_513_inputs(frame):
    """SearchForInitialization with matches all over the frame and ONE F1 keypoint whose 10-px window holds CAND_CAP + 1 F2
    keypoints: the fast path reports the overflow and the exact kernel (the staging pair) computes the call."""
    rng = np.random.default_rng(77)
    kc, dc = cluster(frame, CAND_CAP + 1, rng)
    k0, d0 = kps(frame, 900, rng)
    far = (np.abs(k0["x"] - 900.0) >= 24) | (np.abs(k0["y"] - 500.0) >= 24)
    k0, d0 = k0[far], d0[far]
    k2, d2 = np.concatenate([k0[:700], kc]), np.concatenate([d0[:700], dc])
    k1, d1 = k0[:400].copy(), d0[:400] ^ flips(rng, (400, 32))
    k1["x"] += rng.normal(0, 1.5, 400).astype(np.float32)
    k1["y"] += rng.normal(0, 1.5, 400).astype(np.float32)
    k1["x"][0], k1["y"][0] = 900.0, 500.0
    d1[0] = dc[5] ^ flips(rng, 32, 2)
    k1["octave"] = 0
    k2["octave"] = 0
    return k1, d1, k2, d2, np.stack([k1["x"], k1["y"]], 1).astype(np.float32)


def vocabulary():
    return bs.make_vocabulary(np.random.default_rng(41), k=10, L=3)


def big_local_points_case(pkg, oracle, synth):
    """Tracking::SearchLocalPoints (orbm_search_local_points) on a frame of about 1000 keypoints with the smallest local map whose
    arena passes 4 MiB."""
    n = len(features(oracle, synth.frame(1241, 376, 30 + 7), 1000)[1])
    m = 1
    while arena_need_local_points(n, m) <= ARENA_MIN:
        m += 1
    big = local_points_case(pkg, oracle, synth, m, "search_local_points_big")
    assert big.n == n
    big.need, big.before = arena_need_local_points(n, m), ARENA_MIN
    return big


def local_points_case(pkg, oracle, synth, m, name):
    """Tracking::SearchLocalPoints on that frame with a local map of m world points (m picks the resolver: k_resolve_par with 2 queries
    per thread up to 2048, 4 up to 4096, the single-wave resolver beyond)."""
    ks_, w, h, rng, k, d, sf, cam, log_sf, T, pts3, wp, pd, obs = local_map(pkg, oracle, synth, 7, m=m)
    n = len(k)
    uright = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 40, n), -1).astype(np.float32)
    frame_mp = np.full(n, -1, np.int32)
    held = rng.choice(n, 150, replace=False)
    frame_mp[held[:75]] = rng.choice(len(wp), 75, replace=False)
    frame_mp[held[75:]] = -2
    ext_obs = rng.integers(0, 3, n).astype(np.int32)
    proj = oracle.is_in_frustum(pts3, obs, T, cam, oracle.grid_geom(w, h), 0.5, log_sf, 8)
    on, ofm = oracle.search_by_projection_mp(k, d, uright, oracle.grid_geom(w, h), sf, proj, pd, frame_mp, ext_obs, 1.0, 0.8)
    assert on > 200
    thr = pkg.predict_scale_thresholds(log_sf, 8)
    pcam = pkg.Camera(ks.FX, ks.FY, ks.CX, ks.CY, ks.MBF, np.float32(ks.MBF) / np.float32(ks.FX))

    def run(pkg, shared):
        gn, gfm, gproj = pkg.search_local_points(k, d, uright, pkg.grid_geom(w, h), sf, wp, pd, T, pcam, 0.5, thr, frame_mp, ext_obs, 1.0, 0.8)
        return {"nmatches": gn, "frame_mp": gfm, "projections": np.frombuffer(gproj.tobytes(), np.uint8)}
    case = Case(name, run, {"nmatches": on, "frame_mp": ofm, "projections": np.frombuffer(proj.tobytes(), np.uint8)}, guided=True)
    case.n = n
    return case
