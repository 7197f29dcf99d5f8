"""The scenes of three C++ host-class tests that tests/test_host_cpp_gpu.py runs one at a time and
tests/test_match_threads_host_cpp_gpu.py runs from three threads at once: each writes its input files, and returns the
driver's arguments (between the mode's name and the output prefix) and check(numbers the driver printed, output prefix),
which compares the dumped results with the CPU oracle."""
import numpy as np


def local_points_case(oracle, synth, tmp_path):
    """Tracking::SearchLocalPoints' projection loop + SearchByProjection (src/Tracking.cc:1305-1339,
    src/Frame.cc:284-340) through SearchLocalPointsHIP: one fused GPU call."""
    import kf_scene as ks
    w, h, nf = 1241, 376, 1000
    rng = np.random.default_rng(12)
    img = synth.frame(w, h, 52)
    img.tofile(tmp_path / "a.raw")
    orc = oracle.Extractor(nf, 1.2, 8, 20, 7)
    k, d = orc.extract(img)
    n, m = len(k), 2000
    sf = orc.scale_factors
    log_sf = np.float32(np.log(np.float32(1.2)))
    cam = oracle.Cam(ks.FX, ks.FY, ks.CX, ks.CY, ks.MBF, np.float32(ks.MBF) / np.float32(ks.FX))
    T = ks.pose(rng)
    pts, pd, _ = ks.points_for(oracle, rng, k, d, sf, T, m)
    seen = (rng.random(m) < 0.1).astype(np.int32)
    badp = (rng.random(m) < 0.08) & (seen == 0)
    pts["valid"] = (~badp) & (seen == 0)
    obs = rng.integers(0, 6, m).astype(np.int32)
    uright = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 40, n), -1).astype(np.float32)
    holder = np.full(n, -1, np.int32)
    held = rng.choice(n, 120, replace=False)
    holder[held[:60]] = rng.choice(np.flatnonzero(seen == 1), 60, replace=False)   # points already matched in this frame
    holder[held[60:]] = -2
    ext_obs = rng.integers(0, 3, n).astype(np.int32)
    proj = oracle.is_in_frustum(pts, obs, T, cam, oracle.grid_geom(w, h), 0.5, log_sf, 8)
    on, ofm = oracle.search_by_projection_mp(k, d, uright, oracle.grid_geom(w, h), sf, proj, pd, holder, ext_obs, 3.0, 0.8)
    pts.tofile(tmp_path / "pts.bin"); pd.tofile(tmp_path / "pd.bin")
    with open(tmp_path / "aux.bin", "wb") as f:
        for a in (T, uright, holder, ext_obs, obs, seen):
            f.write(np.ascontiguousarray(a).tobytes())
    camarg = "%r,%r,%r,%r,%r" % (ks.FX, ks.FY, ks.CX, ks.CY, ks.MBF)
    args = [tmp_path / "a.raw", w, h, nf, camarg, tmp_path / "pts.bin", tmp_path / "pd.bin", tmp_path / "aux.bin", 3.0]

    def check(numbers, out):
        out = str(out)
        nk, ret, ntm = numbers
        res = np.fromfile(out + ".i32", np.int32)
        assert nk == n and on > 150
        assert ret == on and ntm == int(proj["in_view"].sum())
        np.testing.assert_array_equal(res[:n], ofm)
        np.testing.assert_array_equal(res[n:], 1 + proj["in_view"])          # IncreaseVisible() exactly for the points in view
    return args, check


def bow_case(oracle, tmp_path):
    """ORBVocabulary::loadFromTextFile / transform (Frame::ComputeBoW, KeyFrame::ComputeBoW) and both
    ORBmatcher::SearchByBoW overloads through the C++ classes, against the DBoW2 / ORBmatcher restatement."""
    import bow_scene as bs
    rng = np.random.default_rng(17)
    voc = bs.make_vocabulary(rng, k=9, L=5, early_leaf=0.03)      # L = 5: ComputeBoW's levelsup = 4 -> nodes of level 1
    ov = oracle.Vocabulary(9, 5, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    bs.write_text(voc, tmp_path / "voc.txt")
    base = bs.features_near_words(rng, voc, 900, noise_bits=4)

    def frame(n):
        nd = n // 7
        src = np.concatenate([rng.permutation(len(base))[:n - nd], rng.integers(0, len(base), nd)])
        rng.shuffle(src)
        noise = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        for _ in range(4):
            noise &= rng.integers(0, 256, (n, 32), dtype=np.uint8)
        r = rng.random(n)
        valid = np.where(r < 0.15, 0, np.where(r < 0.22, 2, 1)).astype(np.uint8)
        return base[src] ^ noise, ((src * 0.4 + rng.normal(0, 4, n)) % 360).astype(np.float32), valid
    d1, a1, v1 = frame(800)
    d2, a2, v2 = frame(850)
    for name, arr in (("d1", d1), ("a1", a1), ("v1", v1), ("d2", d2), ("a2", a2), ("v2", v2)):
        np.ascontiguousarray(arr).tofile(tmp_path / (name + ".bin"))
    ratio = 0.75
    args = [tmp_path / "voc.txt"] + [tmp_path / (x + ".bin") for x in ("d1", "a1", "v1", "d2", "a2", "v2")] + [ratio]

    def check(numbers, out):
        out = str(out)
        n1, n2, nA, nB = numbers
        # BowVector / FeatureVector of keyframe 1
        bw, bv, fv1 = ov.transform(d1, 4)
        bow = np.fromfile(out + ".bow", np.float64).reshape(-1, 2)
        np.testing.assert_array_equal(bow[:, 0].astype(np.int64), bw)
        np.testing.assert_array_equal(bow[:, 1], bv)                              # bit-identical doubles
        raw = np.fromfile(out + ".fv", np.int32)
        got, p = {}, 0
        while p < len(raw):
            got[int(raw[p])] = [int(x) for x in raw[p + 2:p + 2 + raw[p + 1]]]
            p += 2 + raw[p + 1]
        assert got == fv1 and len(fv1) >= 8
        _, _, fv2 = ov.transform(d2, 4)
        nqs, qit, ncs, cit = bs.intersect(fv1, fv2)
        res = np.fromfile(out + ".i32", np.int32)
        # SearchByBoW(KF, F): all candidates, best <= TH_LOW; result indexed by the frame's features
        onA, mA = oracle.search_by_bow(d1, a1, v1 == 1, d2, a2, None, nqs, qit, ncs, cit, 50, 0, ratio, True)
        expectF = np.full(n2, -1, np.int32)
        expectF[mA[mA >= 0]] = np.flatnonzero(mA >= 0)
        assert nA == onA > 100
        np.testing.assert_array_equal(res[:n2], expectF)
        # SearchByBoW(KF1, KF2): candidates need a good map point, best < TH_LOW
        onB, mB = oracle.search_by_bow(d1, a1, v1 == 1, d2, a2, v2 == 1, nqs, qit, ncs, cit, 50, 1, ratio, True)
        assert nB == onB > 80
        np.testing.assert_array_equal(res[n2:], mB)
    return args, check


def triangulation_case(oracle, tmp_path, only_stereo):
    """ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-825) through the C++ class: epipole from the two
    keyframe poses, flags from map points / mvuRight / bOnlyStereo, pairs in increasing first index."""
    import bow_scene as bs
    import kf_scene as ks
    rng = np.random.default_rng(23 + only_stereo)
    voc = bs.make_vocabulary(rng, k=9, L=5, early_leaf=0.03)
    ov = oracle.Vocabulary(9, 5, 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    bs.write_text(voc, tmp_path / "voc.txt")
    base = bs.features_near_words(rng, voc, 900, noise_bits=4)
    pos = np.stack([rng.uniform(20, 1220, len(base)), rng.uniform(20, 356, len(base))], 1)

    def frame(n, dx):
        nd = n // 6
        src = np.concatenate([rng.permutation(len(base))[:n - nd], rng.integers(0, len(base), nd)])
        rng.shuffle(src)
        noise = rng.integers(0, 256, (n, 32), dtype=np.uint8)
        for _ in range(4):
            noise &= rng.integers(0, 256, (n, 32), dtype=np.uint8)
        k = np.zeros(n, oracle.KP_DTYPE)
        k["x"] = pos[src, 0] + dx + rng.normal(0, 0.3, n); k["y"] = pos[src, 1] + rng.normal(0, 0.8, n)
        k["octave"] = rng.integers(0, 8, n); k["angle"] = (src * 0.5 + rng.normal(0, 3, n)) % 360
        has_mp = (rng.random(n) < 0.25).astype(np.uint8)
        ur = np.where(rng.random(n) < 0.5, k["x"] - rng.uniform(1, 30, n), -1).astype(np.float32)
        return base[src] ^ noise, k, has_mp, ur
    d1, k1, m1, u1 = frame(800, 0.0)
    d2, k2, m2, u2 = frame(820, -12.0)
    F12 = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float32)
    T1 = ks.pose(rng); T2 = ks.pose(rng); T2[0, 3] += 0.4
    cam = np.array([ks.FX, ks.FY, ks.CX, ks.CY], np.float32)
    for name, arr in (("d1", d1), ("k1", k1), ("m1", m1), ("u1", u1), ("d2", d2), ("k2", k2), ("m2", m2), ("u2", u2)):
        np.ascontiguousarray(arr).tofile(tmp_path / (name + ".bin"))
    with open(tmp_path / "aux.bin", "wb") as f:
        for a in (F12, T1, T2, cam):
            f.write(np.ascontiguousarray(a, np.float32).tobytes())
    args = [tmp_path / "voc.txt"] + [tmp_path / (x + ".bin") for x in ("d1", "k1", "m1", "u1", "d2", "k2", "m2", "u2")] + [tmp_path / "aux.bin", only_stereo]

    def check(numbers, out):
        out = str(out)
        n1, n2, n = numbers
        # the epipole exactly as :663-670 evaluates it
        Cw = np.array([np.float32(-sum(np.float64(T1[k, i]) * np.float64(T1[k, 3]) for k in range(3))) for i in range(3)], np.float32)
        C2 = np.array([np.float32(sum(np.float64(T2[r, k]) * np.float64(Cw[k]) for k in range(3)) + np.float64(T2[r, 3])) for r in range(3)], np.float32)
        invz = np.float32(1.0) / C2[2]
        ex = cam[0] * C2[0] * invz + cam[2]; ey = cam[1] * C2[1] * invz + cam[3]
        st1, st2 = u1 >= 0, u2 >= 0
        f1 = (((m1 == 0) & (st1 | (only_stereo == 0))).astype(np.uint8)) | (st1.astype(np.uint8) << 1)
        f2 = (((m2 == 0) & (st2 | (only_stereo == 0))).astype(np.uint8)) | (st2.astype(np.uint8) << 1)
        sf = np.ones(8, np.float32)
        for l in range(1, 8):
            sf[l] = sf[l - 1] * np.float32(1.2)
        _, _, fv1 = ov.transform(d1, 4); _, _, fv2 = ov.transform(d2, 4)
        nqs, qit, ncs, cit = bs.intersect(fv1, fv2)
        on, om = oracle.search_for_triangulation(k1, d1, f1, k2, d2, f2, nqs, qit, ncs, cit, F12, ex, ey, sf, sf * sf, 50, False)
        res = np.fromfile(out + ".i32", np.int32).reshape(-1, 2)
        assert n == on > 40 and len(res) == on
        idx = np.flatnonzero(om >= 0)
        np.testing.assert_array_equal(res[:, 0], idx)
        np.testing.assert_array_equal(res[:, 1], om[idx])
    return args, check
