"""GPU: the kernels of csrc/orbx_bow.hip at the shapes where their branches run - nodes with more children than the 16
lanes of a descent group, leaves at every depth of one call, vocabulary nodes with 64 .. 4096 candidates (bits above 0 of
the per-lane `taken` register, runner-up in the winner's lane or in another), the 4096-candidate limit, rotations on bin
edges and histograms at exactly one tenth.  Every result is compared, exactly, with the numpy restatement
tests/bow_ref.py AND with the C oracle (tests/test_bow_cpu.py holds the two to each other without a device), and every
case first asserts on the restatement's `stats` that it reaches the branch it is meant to reach."""
import ctypes as C

import numpy as np
import pytest

import bow_ref
import bow_scene as bs

pytestmark = pytest.mark.gpu


def gpu_bow(pkg, s, variant, ratio, ori):
    v = bs.VARIANTS[variant]
    return pkg.search_by_bow(s["qd"], s["qa"], s["qv"], s["cd"], s["ca"], s["cv"] if v["use_cv"] else None, s["nqs"], s["qit"], s["ncs"],
                             s["cit"], v["max_dist"], ratio, ori)


def gpu_tri(pkg, s, g, ori, max_dist=50):
    return pkg.search_for_triangulation(g["k1"], s["qd"], g["f1"], g["k2"], s["cd"], g["f2"], s["nqs"], s["qit"], s["ncs"], s["cit"],
                                        g["F12"], g["ex"], g["ey"], g["sf"], g["sigma2"], max_dist, ori)


def same(got, want, what=None):
    assert got[0] == want[0], (what, got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1], err_msg=str(what))


# ---- k_voc_descend --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["wide", "deep"])
def test_descent_every_feature(pkg, oracle, name):
    """orbv_transform on the wide vocabulary (1 .. 33 children: up to three steps of the 16-lane stride, planted ties
    across it, a chain of single-child nodes) and on the deep pruned one (k = 10, L = 6, words at every depth 2 .. 6, so
    the lane groups of a wave leave the descent up to four levels apart): word, weight and node of EVERY feature for
    levelsup 0 .. L+1 and every feature count, against bow_ref and the oracle.  Where a path ends above level
    L - levelsup the library's contract is node 0; the reference leaves *nid unset there (bow_ref: None)."""
    voc, feats, paths = bs.descent_case(name)
    late, stride_ties, depths = bs.descent_conditions(name)
    if name == "wide":
        assert late >= 100 and stride_ties >= 1
    else:
        assert depths == [2, 3, 4, 5, 6]
    assert sum(len(nodes) < voc["L"] for nodes, _ in paths) >= 20
    ov = oracle.Vocabulary(voc["k"], voc["L"], 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    gv = pkg.Vocabulary(voc["k"], voc["L"], 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    assert gv.info()["nnodes"] == len(voc["parent"]) and gv.info()["nwords"] == int(voc["is_leaf"].sum())
    words = [bow_ref.word_of(voc, nodes[-1]) for nodes, _ in paths]
    for levelsup in range(voc["L"] + 2):
        nids = [bow_ref.descend(voc, None, levelsup, nodes)[1] for nodes, _ in paths]
        want = (np.array([w for w, _ in words], np.int32), np.array([0 if x is None else x for x in nids], np.int32),
                np.array([x for _, x in words], np.float64))
        for i in range(0, len(feats), 3 if levelsup else 1):            # the oracle too (every feature at levelsup 0)
            assert ov.transform_one(feats[i], levelsup) == (want[0][i], want[2][i], want[1][i]), (levelsup, i)
        for n in bs.FEATURE_COUNTS:
            w, nid, wt = gv.transform(feats[:n], levelsup)
            for got, ref, what in zip((w, nid, wt), want, ("word", "node", "weight")):
                np.testing.assert_array_equal(got, ref[:n], err_msg="%s levelsup %d n %d" % (what, levelsup, n))
    if name == "wide":                                                   # each planted probe takes the planted child
        w, nid, wt = gv.transform(feats[:4], voc["L"] - 2)
        assert list(nid) == [node for _, _, node in voc["probes"]]
    # node_id = NULL and weight = NULL are accepted
    n = 257
    d = np.ascontiguousarray(feats[:n])
    w = np.full(n, -7, np.int32)
    assert gv._L.orbv_transform(gv._h, d.ctypes.data, n, 1, w.ctypes.data, None, None) == 0
    np.testing.assert_array_equal(w, [x for x, _ in words[:n]])


def test_descent_through_the_text_format(pkg, tmp_path):
    """write_text -> Vocabulary(path=...) for the wide vocabulary (header k = 20, up to 33 children on a line's parent) and for
    a regular k = 20 tree: the same answers as the vocabulary built from arrays."""
    voc, feats, paths = bs.descent_case("wide")
    k20 = bs.make_vocabulary(np.random.default_rng(8), k=20, L=2)
    for v, f in ((voc, feats[:600]), (k20, bs.features_near_words(np.random.default_rng(9), k20, 600))):
        bs.write_text(v, tmp_path / "voc.txt")
        tv = pkg.Vocabulary(path=tmp_path / "voc.txt")
        gv = pkg.Vocabulary(v["k"], v["L"], 0, 0, v["parent"], v["is_leaf"], v["desc"], v["weight"])
        assert tv.info() == gv.info() and tv.info()["k"] == 20
        for levelsup in (0, 1, v["L"]):
            a, b = tv.transform(f, levelsup), gv.transform(f, levelsup)
            for x, y in zip(a, b):
                np.testing.assert_array_equal(x, y)
            for i in range(len(f)):
                nodes, _ = paths[i] if v is voc else bow_ref.path(v, f[i])
                leaf, nid = bow_ref.descend(v, None, levelsup, nodes)
                assert (a[0][i], a[2][i]) == bow_ref.word_of(v, leaf) and a[1][i] == (nid or 0)


# ---- k_bow_match ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["kf_frame", "kf_kf"])
def test_search_by_bow_crowded_nodes(pkg, oracle, variant):
    """Nodes of 63, 64, 65, 128, 129, 1000, 4095 and 4096 candidates (and one without candidates, one without queries),
    as 1, 4, 5, 9 and all 10 nodes; ratios 0.7, 0.9, 1.5; rotation filter on and off.  Twice: the same arrays."""
    s = bs.crowded_case()
    assert sorted(np.diff(s["ncs"])) == sorted(bs.CROWD_C) and 0 in np.diff(s["nqs"])
    for ratio in (0.7, 0.9, 1.5):
        rn, rm, st = bs.bow_reference("crowded", variant, ratio)
        assert st["hi"] >= 100 and st["taken_hi"] >= 20                  # winners and taken candidates at positions >= 64
        if ratio == 1.5:
            assert st["ties_across"] >= 10                               # tied pairs in two lanes: the lower position won
        for ori, want in ((True, (rn, rm)), (False, (st["accepted"], st["unfiltered"]))):
            same(bs.oracle_bow(oracle, s, variant, ratio, ori), want, ("oracle", ratio, ori))
            got = gpu_bow(pkg, s, variant, ratio, ori)
            same(got, want, (ratio, ori))
            same(gpu_bow(pkg, s, variant, ratio, ori), got, "second run")
    v = bs.VARIANTS[variant]
    for nnodes in bs.CROWD_NNODES[:-1]:
        t = bs.prefix(s, nnodes)
        want = bow_ref.search_by_bow(t["qd"], t["qa"], t["qv"], t["cd"], t["ca"], t["cv"] if v["use_cv"] else None, t["nqs"], t["qit"],
                                     t["ncs"], t["cit"], v["max_dist"], 0.9, True)
        same(bs.oracle_bow(oracle, t, variant, 0.9, True), want, ("oracle", nnodes))
        same(gpu_bow(pkg, t, variant, 0.9, True), want, nnodes)


@pytest.mark.parametrize("variant", ["kf_frame", "kf_kf"])
def test_search_by_bow_planted_pairs(pkg, oracle, variant):
    """Best and runner-up planted at chosen positions and distances of a 4096-candidate node: in one lane (p and
    p + 64 m, either order) and in two, accepted and refused by the ratio ((30, 40) and (27, 36) at exactly 0.75), tied
    (the lower position wins, accepted only above ratio 1), d1 == max_dist and max_dist + 1, a sole candidate at
    distance 256, invalid candidates that are neither match nor runner-up."""
    s, index = bs.planted_case(bs.VARIANTS[variant]["max_dist"])
    for ratio in (0.7, 0.75, 0.9, 1.5):
        rn, rm, st = bs.bow_reference("planted", variant, ratio)
        assert st["same_lane"] >= 10 and st["other_lane"] >= 10
        if ratio == 1.5:
            assert st["ties_across"] >= 10
        assert {k: sum(int(rm[i] >= 0) for i in ix) for k, ix in index.items()} == bs.planted_answers(variant, ratio)
        same(bs.oracle_bow(oracle, s, variant, ratio, True), (rn, rm), ("oracle", ratio))
        same(gpu_bow(pkg, s, variant, ratio, True), (rn, rm), ratio)


# ---- the 4096-candidate limit -----------------------------------------------------------------------------------------
def _raw(pkg, entry, s, g):
    """The C entry point itself: the Python wrapper raises before it returns match_q.  -> (rc, match_q, nmatches)"""
    p = lambda a: None if a is None else np.ascontiguousarray(a).ctypes.data
    mq, n = np.full(len(s["qa"]), 7, np.int32), C.c_int(5)
    if entry == "search_by_bow":
        rc = pkg.lib().orbm_search_by_bow(p(s["qd"]), p(s["qa"]), p(s["qv"]), len(s["qa"]), p(s["cd"]), p(s["ca"]), None, len(s["ca"]),
                                          p(s["nqs"]), p(s["qit"]), p(s["ncs"]), p(s["cit"]), len(s["nqs"]) - 1, 50, 0.9, 1, mq.ctypes.data,
                                          C.byref(n), 0)
    else:
        rc = pkg.lib().orbm_search_for_triangulation(p(g["k1"]), p(s["qd"]), p(g["f1"]), len(g["k1"]), p(g["k2"]), p(s["cd"]), p(g["f2"]),
                                                     len(g["k2"]), p(s["nqs"]), p(s["qit"]), p(s["ncs"]), p(s["cit"]), len(s["nqs"]) - 1,
                                                     p(g["F12"]), g["ex"], g["ey"], p(g["sf"]), p(g["sigma2"]), 8, 50, 1, mq.ctypes.data,
                                                     C.byref(n), 0)
    return rc, mq, n.value


@pytest.mark.parametrize("entry", ["search_by_bow", "search_for_triangulation"])
def test_candidate_limit_per_node(pkg, oracle, entry):
    """4096 candidates in a node is served (the crowded cases hold it to the reference); 4097 is ORBX_ERR_UNSUPPORTED
    by design - the wave leaves before it reads a candidate - with match_q all -1 and nmatches 0, and the next ordinary
    call on the same thread is right."""
    big = bs.crowded_nodes((6, 5, 4), (70, 4097, 9), 31)
    gb = bs.tri_geometry(big, 32)
    rc, mq, n = _raw(pkg, entry, big, gb)
    assert rc == pkg.ORBX_ERR_UNSUPPORTED and "4096" in pkg.lib().orbx_last_error().decode()
    assert (mq == -1).all() and n == 0
    with pytest.raises(pkg.OrbxError) as e:
        gpu_bow(pkg, big, "kf_frame", 0.9, True) if entry == "search_by_bow" else gpu_tri(pkg, big, gb, True)
    assert e.value.status == pkg.ORBX_ERR_UNSUPPORTED
    ok = bs.crowded_nodes((6, 5, 4), (70, 4096, 9), 31)
    go = bs.tri_geometry(ok, 32)
    if entry == "search_by_bow":
        want = bs.oracle_bow(oracle, ok, "kf_frame", 0.9, True)
        same(bow_ref.search_by_bow(ok["qd"], ok["qa"], ok["qv"], ok["cd"], ok["ca"], None, ok["nqs"], ok["qit"], ok["ncs"], ok["cit"], 50,
                                   0.9)[:2], want)
        same(gpu_bow(pkg, ok, "kf_frame", 0.9, True), want)
    else:
        want = bs.oracle_tri(oracle, ok, go, True)
        same(bow_ref.search_for_triangulation(go["k1"], ok["qd"], go["f1"], go["k2"], ok["cd"], go["f2"], ok["nqs"], ok["qit"], ok["ncs"],
                                              ok["cit"], go["F12"], go["ex"], go["ey"], go["sf"], go["sigma2"])[:2], want)
        same(gpu_tri(pkg, ok, go, True), want)
    assert want[0] > 0
    rc, mq, n = _raw(pkg, entry, ok, go)
    assert rc == 0 and n == want[0]


# ---- k_bow_orient / three_maxima -------------------------------------------------------------------------------------
def _bin(qa, ca):
    """The reference's bin of one rotation in np.float32 arithmetic (round(): halves away from zero)."""
    f = np.float32
    rot = f(qa) - f(ca)
    if rot < 0.0:
        rot = rot + f(360.0)
    x = rot * (f(1.0) / f(30))
    assert type(x) is np.float32
    lo = np.floor(x)
    b = int(lo) + int(x - lo >= f(0.5))                                  # x - floor(x) is exact
    return 0 if b == 30 else b


def test_rotation_histograms(pkg, oracle):
    """Histograms fixed pair by pair (one identical query and candidate per node, nq > 256): (50, 50, 5), (10, 10, 1) and
    (70, 7, 7) keep the bin at exactly one tenth, (50, 50, 4) and (70, 6, 6) do not; four equal bins keep the first three;
    one bin; no match; rotations on the bin edges 15, 45, .. 345, at -0.0, wrapping from below zero to just under 360
    and to 360 itself, and the bin 30 -> 0 rule.  nmatches and the surviving set are exact, through both entry points."""
    for c in bs.orientation_cases():
        s, name = c["scene"], c["name"]
        for qa, ca, want in c["planted"]:
            assert _bin(qa, ca) == want, (name, qa, ca)
        rn, rm, st = bow_ref.search_by_bow(s["qd"], s["qa"], s["qv"], s["cd"], s["ca"], None, s["nqs"], s["qit"], s["ncs"], s["cit"], 50, 0.7)
        assert (st["histogram"] == c["hist"]).all() and rn == c["nmatches"] and len(s["qa"]) > 256, name
        same(bs.oracle_bow(oracle, s, "kf_frame", 0.7, True), (rn, rm), ("oracle", name))
        same(gpu_bow(pkg, s, "kf_frame", 0.7, True), (rn, rm), name)
        unfiltered = gpu_bow(pkg, s, "kf_frame", 0.7, False)
        same(unfiltered, (st["accepted"], st["unfiltered"]), name)
        g = bs.singleton_tri(s)
        g["f1"][s["qv"] == 0] = 0
        same(bs.oracle_tri(oracle, s, g, True), (rn, rm), ("oracle tri", name))
        same(gpu_tri(pkg, s, g, True), (rn, rm), ("tri", name))


# ---- k_tri_match ----------------------------------------------------------------------------------------------------
def test_search_for_triangulation_crowded_nodes(pkg, oracle):
    """The crowded node sizes with half of each node's candidates exact copies of another one: the minimum distance is
    shared by several candidates that pass the geometric tests, and the LAST in list order wins - at positions >= 64.
    Monocular and stereo features on both sides, unusable queries and candidates among the usable ones."""
    s, g = bs.tri_case()
    rn, rm, st = bs.tri_reference()
    assert st["shared_last_hi"] >= 50 and st["taken_hi"] >= 20
    for side in (g["f1"], g["f2"]):
        assert all((side == v).sum() > 20 for v in (0, 1, 2, 3))
    for ori, want in ((True, (rn, rm)), (False, (st["accepted"], st["unfiltered"]))):
        same(bs.oracle_tri(oracle, s, g, ori), want, ("oracle", ori))
        got = gpu_tri(pkg, s, g, ori)
        same(got, want, ori)
        same(gpu_tri(pkg, s, g, ori), got, "second run")
    for nnodes in bs.CROWD_NNODES[:-1]:
        t = bs.prefix(s, nnodes)
        want = bs.oracle_tri(oracle, t, g, True)
        same(bow_ref.search_for_triangulation(g["k1"], t["qd"], g["f1"], g["k2"], t["cd"], g["f2"], t["nqs"], t["qit"], t["ncs"], t["cit"],
                                              g["F12"], g["ex"], g["ey"], g["sf"], g["sigma2"])[:2], want, ("ref", nnodes))
        same(gpu_tri(pkg, t, g, True), want, nnodes)


def test_search_for_triangulation_edges(pkg, oracle):
    """One float step on either side of each comparison: a candidate exactly 10 px from the epipole at octave 0 is kept
    (100 < 100 is false), one step nearer is dropped unless a side is stereo; the last y2 with dsqr < 3.84 sigma2 and the
    next one, on both sides of the line; den == 0, den that underflows to 0, a subnormal den and the smallest normal."""
    for c in bs.tri_edge_cases():
        s, g, name = c["scene"], c["geom"], c["name"]
        rn, rm, _ = bow_ref.search_for_triangulation(g["k1"], s["qd"], g["f1"], g["k2"], s["cd"], g["f2"], s["nqs"], s["qit"], s["ncs"],
                                                     s["cit"], g["F12"], g["ex"], g["ey"], g["sf"], g["sigma2"])
        assert [bool(rm[i] >= 0) for i in s["pair_q"]] == c["expect"], name
        same(bs.oracle_tri(oracle, s, g, True), (rn, rm), ("oracle", name))
        same(gpu_tri(pkg, s, g, True), (rn, rm), name)
