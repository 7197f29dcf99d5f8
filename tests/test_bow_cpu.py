"""CPU: the C oracle of the DBoW2 descent and the BoW-guided matchers (oracle/orb_oracle_bow.c) against the numpy
restatement tests/bow_ref.py, on every case tests/test_bow_gpu.py runs on the device - so the GPU results are held to
a reference that two independent texts of src/ORBmatcher.cc and TemplatedVocabulary.h agree on - plus the coverage
conditions of those cases (which branch of the wave-per-node kernels each one reaches) and the argument checks of
orbm_search_by_bow / orbm_search_for_triangulation that need no device.  Everything is exact: integers only."""
import ctypes as C

import numpy as np
import pytest

import bow_ref
import bow_scene as bs


def test_descent_cases_reach_their_branches():
    late, stride_ties, _ = bs.descent_conditions("wide")
    assert late >= 100                                       # path steps through a child position >= 16
    assert stride_ties >= 1                                  # a step decided by a tie across the 16-stride
    voc, feats, paths = bs.descent_case("wide")
    counts = np.bincount(voc["parent"][1:], minlength=len(voc["parent"]))
    assert set(counts) == set(bs.WIDE_COUNTS) | {0, 20} and (counts[voc["parent"][counts == 1]] == 1).sum() >= 2   # a chain
    for i, (name, probe, node) in enumerate(voc["probes"]):
        nodes, steps = paths[i]
        assert (feats[i] == probe).all() and nodes[1] == node, name
    tied = {name: [int(t) for t in paths[i][1][1][1]] for i, (name, _, _) in enumerate(voc["probes"])}
    assert tied == {"tie_2_18": [2, 18], "tie_0_16": [0, 16], "best_17": [17], "best_33rd": [32]}
    voc, feats, paths = bs.descent_case("deep")
    assert len(voc["parent"]) < 40000
    _, _, depths = bs.descent_conditions("deep")
    assert depths == [2, 3, 4, 5, 6]                         # words reached at every depth in one call
    assert sum(len(nodes) < voc["L"] for nodes, _ in paths) >= 20      # paths that end above the nid level of levelsup 0


@pytest.mark.parametrize("name", ["wide", "deep"])
def test_descent_oracle_is_the_restatement(oracle, name):
    """oracle_voc_transform_one == bow_ref.descend + word_of for every feature and levelsup 0 .. L+1.  Where the path
    ends above level L - levelsup the reference leaves *nid unset (bow_ref: None); the oracle's caller and the library
    report 0."""
    voc, feats, paths = bs.descent_case(name)
    ov = oracle.Vocabulary(voc["k"], voc["L"], 0, 0, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"])
    unset = 0
    for levelsup in range(voc["L"] + 2):
        for i in range(0, len(feats), 1 if levelsup in (0, 2) else 5):
            leaf, nid = bow_ref.descend(voc, feats[i], levelsup, paths[i][0])
            unset += nid is None
            word, weight = bow_ref.word_of(voc, leaf)
            assert ov.transform_one(feats[i], levelsup) == (word, weight, 0 if nid is None else nid), (levelsup, i)
    assert unset >= 20
    leaf, nid = bow_ref.descend(voc, feats[7], 1)            # without a precomputed path
    assert (leaf, nid) == bow_ref.descend(voc, feats[7], 1, paths[7][0])


@pytest.mark.parametrize("variant", ["kf_frame", "kf_kf"])
def test_crowded_oracle_is_the_restatement(oracle, variant):
    s = bs.crowded_case()
    assert (s["cit"] != np.arange(len(s["cit"]))).mean() > 0.9 and (s["qit"] != np.arange(len(s["qit"]))).mean() > 0.9
    for ratio in (0.7, 0.9, 1.5):
        rn, rm, st = bs.bow_reference("crowded", variant, ratio)
        assert st["hi"] >= 100 and st["taken_hi"] >= 20
        on, om = bs.oracle_bow(oracle, s, variant, ratio, True)
        assert on == rn and (om == rm).all()
        on, om = bs.oracle_bow(oracle, s, variant, ratio, False)
        assert on == st["accepted"] and (om == st["unfiltered"]).all()
    v = bs.VARIANTS[variant]                                 # stats["unfiltered"] IS the answer without the rotation filter
    t = bs.prefix(s, 4)
    rn, rm, st = bow_ref.search_by_bow(t["qd"], t["qa"], t["qv"], t["cd"], t["ca"], t["cv"] if v["use_cv"] else None, t["nqs"], t["qit"],
                                       t["ncs"], t["cit"], v["max_dist"], 0.9, False)
    assert rn == st["accepted"] and (rm == st["unfiltered"]).all() and "histogram" not in st
    on, om = bs.oracle_bow(oracle, t, variant, 0.9, False)
    assert on == rn and (om == rm).all()


@pytest.mark.parametrize("variant", ["kf_frame", "kf_kf"])
def test_planted_oracle_is_the_restatement(oracle, variant):
    """Known answers of the planted pairs, on the restatement and on the oracle."""
    s, index = bs.planted_case(bs.VARIANTS[variant]["max_dist"])
    for ratio in (0.7, 0.75, 0.9, 1.5):
        rn, rm, st = bs.bow_reference("planted", variant, ratio)
        on, om = bs.oracle_bow(oracle, s, variant, ratio, True)
        assert on == rn and (om == rm).all()
        assert st["same_lane"] >= 10 and st["other_lane"] >= 10
        got = {k: sum(int(rm[i] >= 0) for i in ix) for k, ix in index.items()}
        assert got == bs.planted_answers(variant, ratio), ratio
        if ratio == 1.5:
            assert st["ties_across"] >= 10 and st["ties"] > st["ties_across"]


def test_tri_oracle_is_the_restatement(oracle):
    s, g = bs.tri_case()
    rn, rm, st = bs.tri_reference()
    assert st["shared_last_hi"] >= 50 and st["hi"] >= 100 and st["taken_hi"] >= 20
    assert ((g["f1"] & 1) == 0).sum() > 20 and ((g["f2"] & 1) == 0).sum() > 20          # unusable among usable, both sides
    for ori, n, m in ((True, rn, rm), (False, st["accepted"], st["unfiltered"])):
        on, om = bs.oracle_tri(oracle, s, g, ori)
        assert on == n and (om == m).all()


def test_orientation_cases_oracle_is_the_restatement(oracle):
    """The planted histograms come out as planned (bins, sizes, survivors) on the restatement, and the oracle agrees."""
    for c in bs.orientation_cases():
        s = c["scene"]
        assert all(bow_ref.rotation_bin(a, b) == want for a, b, want in c["planted"]), c["name"]
        rn, rm, st = bow_ref.search_by_bow(s["qd"], s["qa"], s["qv"], s["cd"], s["ca"], None, s["nqs"], s["qit"], s["ncs"], s["cit"], 50, 0.7)
        assert (st["histogram"] == c["hist"]).all() and rn == c["nmatches"], c["name"]
        on, om = bs.oracle_bow(oracle, s, "kf_frame", 0.7, True)
        assert on == rn and (om == rm).all(), c["name"]
        g = bs.singleton_tri(s)
        g["f1"][s["qv"] == 0] = 0
        tn, tm, _ = bow_ref.search_for_triangulation(g["k1"], s["qd"], g["f1"], g["k2"], s["cd"], g["f2"], s["nqs"], s["qit"], s["ncs"],
                                                     s["cit"], g["F12"], g["ex"], g["ey"], g["sf"], g["sigma2"])
        assert tn == rn and (tm == rm).all(), c["name"]
        on, om = bs.oracle_tri(oracle, s, g, True)
        assert on == rn and (om == rm).all(), c["name"]


def test_tri_edge_cases_oracle_is_the_restatement(oracle):
    for c in bs.tri_edge_cases():
        s, g = c["scene"], c["geom"]
        rn, rm, _ = bow_ref.search_for_triangulation(g["k1"], s["qd"], g["f1"], g["k2"], s["cd"], g["f2"], s["nqs"], s["qit"], s["ncs"],
                                                     s["cit"], g["F12"], g["ex"], g["ey"], g["sf"], g["sigma2"])
        assert [bool(rm[i] >= 0) for i in s["pair_q"]] == c["expect"], c["name"]
        assert all(rm[q] in (-1, p) for q, p in zip(s["pair_q"], s["pair_c"]))
        on, om = bs.oracle_tri(oracle, s, g, True)
        assert on == rn and (om == rm).all(), c["name"]


def test_three_maxima_known_answers(oracle):
    """ComputeThreeMaxima: `max3 < 0.1f*(float)max1` is FALSE at exactly one tenth (the float product is the integer),
    ties keep the earlier bins."""
    def h(**bins):
        x = [0] * 30
        for k, v in bins.items():
            x[int(k[1:])] = v
        return x
    cases = [(h(b3=50, b7=50, b9=5), (3, 7, 9)), (h(b3=50, b7=50, b9=4), (3, 7, -1)), (h(b3=10, b7=10, b9=1), (3, 7, 9)),
             (h(b3=70, b7=7, b9=7), (3, 7, 9)), (h(b3=70, b7=6, b9=7), (3, 9, -1)), (h(b3=70, b7=6, b9=6), (3, -1, -1)),
             (h(b2=30, b5=30, b11=30, b29=30), (2, 5, 11)), (h(b29=1), (29, -1, -1)), ([0] * 30, (-1, -1, -1))]
    for hist, want in cases:
        assert bow_ref.three_maxima(hist) == want and oracle.three_maxima(hist) == want, hist
    rng = np.random.default_rng(0)
    for _ in range(300):
        hist = list(rng.integers(0, rng.integers(1, 60), 30))
        assert bow_ref.three_maxima(hist) == oracle.three_maxima(hist)


def test_rotation_bins():
    """The bin arithmetic in float: bin 1 starts one step BELOW 15 degrees (there rot * (1.0f/30) already rounds to 0.5f, and halves go up),
    -0.0 stays in bin 0, a negative difference wraps to just under 360 (bin 12 -> 12, 360 itself -> 12), bin 30 -> 0."""
    f = np.float32
    edge = f(14.99)
    while bow_ref.rotation_bin(edge, 0) == 0:
        edge = np.nextafter(edge, f(16))
    assert edge == np.nextafter(f(15), f(0)) and bow_ref.rotation_bin(15, 0) == 1     # the product rounds up to 0.5f one step early
    assert bow_ref.rotation_bin(-0.0, 0.0) == 0 and bow_ref.rotation_bin(0, 1e-6) == 12 and bow_ref.rotation_bin(0, 1) == 12
    assert bow_ref.rotation_bin(900, 0) == 0 and bow_ref.rotation_bin(884, 0) == 29


# ---- argument checks of the product library: no device is needed, they come before any HIP call -----------------------
def _bow_call(pkg, s, nq_items, nc_items):
    mq = np.full(len(s["qa"]), 7, np.int32)
    n = C.c_int(5)
    p = lambda a: np.ascontiguousarray(a).ctypes.data
    rc = pkg.lib().orbm_search_by_bow(p(s["qd"]), p(s["qa"]), p(s["qv"]), len(s["qa"]), p(s["cd"]), p(s["ca"]), None, len(s["ca"]),
                                      p(s["nqs"]), p(nq_items), p(s["ncs"]), p(nc_items), len(s["nqs"]) - 1, 50, 0.7, 1,
                                      mq.ctypes.data, C.byref(n), 0)
    return rc, mq, n.value


def _tri_call(pkg, s, g, nq_items, nc_items):
    mq = np.full(len(g["k1"]), 7, np.int32)
    n = C.c_int(5)
    p = lambda a: np.ascontiguousarray(a).ctypes.data
    rc = pkg.lib().orbm_search_for_triangulation(p(g["k1"]), p(s["qd"]), p(g["f1"]), len(g["k1"]), p(g["k2"]), p(s["cd"]), p(g["f2"]),
                                                 len(g["k2"]), p(s["nqs"]), p(nq_items), p(s["ncs"]), p(nc_items), len(s["nqs"]) - 1,
                                                 p(g["F12"]), 600.0, 180.0, p(g["sf"]), p(g["sigma2"]), 8, 50, 1, mq.ctypes.data,
                                                 C.byref(n), 0)
    return rc, mq, n.value


@pytest.mark.parametrize("entry", ["search_by_bow", "search_for_triangulation"])
@pytest.mark.parametrize("side", ["q_items", "c_items"])
def test_repeated_feature_index_is_an_argument_error(pkg, entry, side):
    """include/orbx.h: a feature belongs to one node only.  An index listed twice - in one node or in two - is
    ORBX_ERR_ARG with a message, match_q all -1 and *nmatches 0; found on the host, so this needs no GPU."""
    s = bs.crowded_nodes((3, 2, 4), (5, 3, 2), 1)
    g = bs.tri_geometry(s, 2)
    for i, j in ((0, 1), (0, len(s[side[0] + "it"]) - 1)):      # twice in the first node; in the first and in the last
        qit, cit = s["qit"].copy(), s["cit"].copy()
        items = qit if side == "q_items" else cit
        items[j] = items[i]
        rc, mq, n = _bow_call(pkg, s, qit, cit) if entry == "search_by_bow" else _tri_call(pkg, s, g, qit, cit)
        assert rc == pkg.ORBX_ERR_ARG
        msg = pkg.lib().orbx_last_error().decode()
        assert entry in msg and "%s[%d] repeats feature %d" % (side, j, items[j]) in msg, msg
        assert (mq == -1).all() and n == 0
