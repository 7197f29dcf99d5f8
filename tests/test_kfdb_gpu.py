"""GPU: the keyframe database (orbv_db_*, orb_slam2v2-1_amd/csrc/orbx_kfdb.hip) against the restatement tests/kfdb_ref.py,
field for field: candidates, the records of the listed keyframes (floats bit-equal) and orbv_db_score's doubles (bit-equal).
Every case asserts on the restatement's trace that it reaches the branch it was built for."""
import ctypes as C
import os
import sys
import threading

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kfdb_ref as R        # noqa: E402
import kfdb_scene as S      # noqa: E402

pytestmark = pytest.mark.gpu
F = np.float32


def f32bits(x):
    return int(np.array([x], np.float32).view(np.uint32)[0])


def f64bits(x):
    return int(np.array([x], np.float64).view(np.uint64)[0])


def same_hits(got, want):
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        assert (int(g["kf_id"]), int(g["words"]), int(g["flags"]), int(g["best_kf"])) == (w[0], w[1], w[2], w[5]), (g, w)
        assert f32bits(g["score"]) == f32bits(w[3]) and f32bits(g["acc_score"]) == f32bits(w[4]), (g, w)


class Pair:
    """the library's database and the restatement, fed the same calls"""

    def __init__(self, pkg, nwords, initial_entries=0):
        self.db = pkg.KeyFrameDatabase(nwords, initial_entries=initial_entries)
        self.ref = R.Session(nwords)

    def add(self, kf_id, v):
        self.db.add(kf_id, *S.arrays(v)); self.ref.add(kf_id, v)

    def erase(self, kf_id):
        self.db.erase(kf_id); self.ref.erase(kf_id)

    def clear(self):
        self.db.clear(); self.ref.clear()

    def cov(self, kf_id, ids):
        self.db.set_covisible(kf_id, ids); self.ref.set_covisible(kf_id, ids)

    def fill(self, kfs, cov=None):
        for i in kfs:
            self.add(i, kfs[i])
        for i, c in (cov or {}).items():
            self.cov(i, c)

    def reloc(self, q):
        cand, hits = self.db.detect_relocalization_candidates(*S.arrays(q), hits=True)
        rc, rh, t = self.ref.detect_reloc(q)
        same_hits(hits, rh)
        assert list(cand) == rc
        return t

    def loop(self, q, connected, min_score):
        cand, hits = self.db.detect_loop_candidates(*S.arrays(q), connected, min_score, hits=True)
        rc, rh, t = self.ref.detect_loop(q, connected, min_score)
        same_hits(hits, rh)
        assert list(cand) == rc
        return t

    def score(self, q, ids):
        got = self.db.score(*S.arrays(q), ids)
        assert [f64bits(x) for x in got] == [f64bits(x) for x in self.ref.score(q, ids)]
        return got


def ids_of(kfs):
    return [k.mnId for k in kfs]


NW = 20000


@pytest.fixture(scope="module")
def lengths_pair(pkg):
    """keyframe vectors of 0, 1, 63, 64, 65, 129 and 1500 words (ids 1..7) and two more long ones"""
    rng = np.random.default_rng(21)
    p = Pair(pkg, NW)
    kfs = {i + 1: S.random_bow(rng, NW, n) for i, n in enumerate([0, 1, 63, 64, 65, 129, 1500, 1480, 1520])}
    p.fill(kfs, {7: [8, 9, 3], 8: [7], 4: [5, 6, 7]})
    return p, kfs


@pytest.mark.parametrize("nq", [1, 64, 65, 2000, 8192])
def test_vector_and_query_lengths(pkg, lengths_pair, nq):
    p, kfs = lengths_pair
    assert nq <= pkg.DB_MAX_QUERY
    q = S.overlapping_query(np.random.default_rng(100 + nq), NW, [kfs[i] for i in (2, 3, 4, 5, 6)] + ([kfs[7]] if nq > 100 else []), nq)
    assert len(q) == nq
    s = p.score(q, sorted(kfs))
    assert f64bits(s[0]) == f64bits(-0.0)                     # the empty keyframe
    t = p.reloc(q)
    assert len(t["listed"]) >= 1 and 1 not in ids_of(t["listed"])
    t = p.loop(q, [], 0.0)
    if nq >= 64:
        assert len(t["listed"]) >= 5 and len(t["scored"]) < len(t["listed"])


def test_query_above_the_bound_is_unsupported(pkg, lengths_pair):
    p, _ = lengths_pair
    w = np.arange(pkg.DB_MAX_QUERY + 1, dtype=np.uint32); v = np.full(len(w), 1.0 / len(w))
    for call in (lambda: p.db.detect_relocalization_candidates(w, v), lambda: p.db.detect_loop_candidates(w, v, [], 0.0),
                 lambda: p.db.score(w, v, [2])):
        with pytest.raises(pkg.OrbxError) as e:
            call()
        assert e.value.status == pkg.ORBX_ERR_UNSUPPORTED


def test_common_words_at_chunk_edges(pkg):
    """a wave walks a keyframe's entries 64 at a time: common words only in the last lane of the first chunk, only in the first
    lane of the second, and in every chunk"""
    rng = np.random.default_rng(22)
    p = Pair(pkg, 4000)
    words = list(range(0, 1300, 10))                          # 130 entries: chunks of 64, 64, 2
    for i in range(1, 6):
        p.add(i, S.bow(rng, words))
    p.add(6, S.bow(rng, words[:64]))
    p.add(7, S.bow(rng, words[:65]))
    p.cov(1, [2, 6]); p.cov(6, [7, 1])
    other = list(range(5, 1300, 10))
    for pos in ([63], [64], [5, 70, 129], [0], [129], [63, 64], list(range(130))):
        q = S.bow(rng, [words[k] for k in pos] + other[:40])
        t = p.reloc(q)
        want = [i for i in range(1, 8) if any(k < len(p.ref.kf[i].mBowVec) for k in pos)]
        assert ids_of(t["listed"]) == want and t["maxCommonWords"] == len(pos)
        p.loop(q, [2], 0.0)
        p.score(q, list(range(1, 8)))


@pytest.mark.parametrize("nkf", [1, 4, 5, 257])
def test_keyframe_counts(pkg, nkf):
    """1, 4, 5: edges of four waves per workgroup; 257: one more than a pass of k_db_select"""
    rng = np.random.default_rng(23 + nkf)
    p = Pair(pkg, 300)
    kfs, cov = S.crowd(rng, 300, nkf, 40, absent_id=9999)
    p.fill(kfs, cov)
    for k in range(3):
        q = S.random_bow(rng, 300, 60)
        t = p.reloc(q)
        assert len(t["listed"]) == nkf or nkf == 1
        t = p.loop(q, [int(i) for i in rng.choice(sorted(kfs), nkf // 3, replace=False)], 0.01)
        assert len(t["listed"]) == nkf - nkf // 3 or nkf == 1
    if nkf == 257:
        assert len(t["entries"]) > 3 and any(len(p.ref.cov[k.mnId]) > 0 for _, k in t["entries"])
    p.score(q, sorted(kfs))


@pytest.mark.parametrize("max_common,min_common", [(5, 4), (10, 8)])
def test_threshold_edges(pkg, max_common, min_common):
    rng = np.random.default_rng(24)
    qwords = list(range(0, 2 * max_common, 2))
    q = S.bow(rng, qwords)
    p = Pair(pkg, 400)
    counts = [min_common, max_common, min_common, min_common + 1, min_common, min_common + 1, 1]
    for k, nc in enumerate(counts):
        p.add(k + 1, S.with_common(rng, qwords, nc, list(range(101 + 10 * k, 400)), 7))
    p.cov(2, [1, 4, 3])
    for t in (p.reloc(q), p.loop(q, [], 0.0)):
        assert (t["maxCommonWords"], t["minCommonWords"]) == (max_common, min_common)
        assert ids_of(t["scored"]) == [2, 4, 6]


def test_loop_connected_set(pkg):
    rng = np.random.default_rng(25)
    qwords = list(range(0, 40, 2))                            # 20 query words
    q = S.bow(rng, qwords)
    p = Pair(pkg, 1000)
    for k, nc in enumerate([20, 5, 5, 4, 5, 3]):              # keyframe 1 would have had the most common words
        p.add(k + 1, S.with_common(rng, qwords, nc, list(range(101 + 20 * k, 1000)), 9))
    p.cov(2, [1, 3, 5]); p.cov(3, [1]); p.cov(5, [6, 1, 2])
    t = p.loop(q, [], 0.0)
    assert t["maxCommonWords"] == 20 and ids_of(t["scored"]) == [1]
    t = p.loop(q, [1, 777], 0.0)                              # 777: a connected keyframe the database does not hold
    assert t["maxCommonWords"] == 5 and t["minCommonWords"] == 4 and 1 not in ids_of(t["listed"])
    assert ids_of(t["scored"]) == [2, 3, 5]
    # keyframe 1 is a neighbour of listed entries and does not count: 2's accumulation holds 3 and 5 only
    acc2 = [a for (si, k), a in zip(t["entries"], t["acc"]) if k.mnId == 2][0][0]
    s = {k.mnId: si for si, k in t["entries"]}
    assert f32bits(acc2) == f32bits(F(F(s[2] + s[3]) + s[5]))
    t = p.loop(q, [], 0.0)                                    # the flags were cleared: 1 is back
    assert ids_of(t["scored"]) == [1]


def test_loop_score_edges(pkg):
    rng = np.random.default_rng(26)
    qwords = list(range(0, 20, 2))
    q = S.bow(rng, qwords)
    p = Pair(pkg, 1000)
    for k in range(8):
        p.add(k + 1, S.with_common(rng, qwords, 10 if k % 2 else 9, list(range(101 + 20 * k, 1000)), 3 + 5 * k))
    for k in range(8):
        p.cov(k + 1, [(k + 1) % 8 + 1, (k + 4) % 8 + 1])
    t = p.loop(q, [], 0.0)
    scores = sorted(si for si, _ in t["entries"])
    assert len(scores) == 8 and len(set(scores)) == 8
    min_score = scores[4]                                      # a float a keyframe scores exactly
    t = p.loop(q, [], float(min_score))
    entered = [k.mnId for _, k in t["entries"]]
    assert len(entered) == 4 and min(si for si, _ in t["entries"]) == min_score          # si == minScore is kept
    low = [k.mnId for k in t["scored"] if k.mLoopScore < min_score]
    assert any(n in low for e in entered for n in p.ref.cov[e])                          # a neighbour below minScore adds


def test_selection_edges(pkg):
    rng = np.random.default_rng(27)
    # two entries whose best keyframe is the same neighbour: one candidate, at the first entry's position
    qwords = list(range(0, 20, 2))
    q = S.bow(rng, qwords)
    p = Pair(pkg, 1000)
    p.add(1, S.with_common(rng, qwords, 10, list(range(100, 1000)), 30))
    p.add(2, S.with_common(rng, qwords, 10, list(range(200, 1000)), 25))
    p.add(3, [(w, x) for w, x in q])                          # the query itself: score 1
    p.add(4, S.with_common(rng, qwords, 9, list(range(300, 1000)), 40))
    p.cov(1, [3]); p.cov(2, [4, 3])
    for t in (p.reloc(q), p.loop(q, [], 0.0)):
        assert [k.mnId for _, k in t["acc"]] == [3, 3, 3, 4]
    cand = p.db.detect_relocalization_candidates(*S.arrays(q))
    assert list(cand).count(3) == 1 and cand[0] == 3
    # acc == 0.75f * bestAcc is not retained: exact binary values (unnormalised vectors are legal input)
    p = Pair(pkg, 16)
    q = [(0, 0.5), (1, 0.375), (2, 0.3750001), (3, 0.25)]
    p.add(1, [(1, 0.375)]); p.add(2, [(0, 0.5)]); p.add(3, [(2, 0.3750001)]); p.add(4, [(3, 0.25), (9, 0.5)])
    for t, ret in ((p.reloc(q), F(0.375)), (p.loop(q, [], 0.1), F(0.375))):
        assert t["minScoreToRetain"] == ret and [a for a, _ in t["acc"]][1] == ret
        assert [a > t["minScoreToRetain"] for a, _ in t["acc"]] == [True, False, True, False]
    assert list(p.db.detect_relocalization_candidates(*S.arrays(q))) == [2, 3]


def test_reloc_stale_fresh_and_absent_neighbours(pkg):
    rng = np.random.default_rng(28)
    p = Pair(pkg, 2000)
    wa, wb = list(range(0, 40, 2)), list(range(1000, 1040, 2))
    qa, qb = S.bow(rng, wa + [1100]), S.bow(rng, wb)
    n_words = wa[:18] + [1000] + list(range(500, 520))        # N: 18 words of query A, one word of query B
    m_words = [1002] + list(range(600, 620))                  # M: one word of query B, none of A
    p.add(1, S.bow(rng, n_words)); p.add(2, S.bow(rng, m_words))
    p.add(3, S.bow(rng, wb[:19] + list(range(700, 730))))      # E: scored by B
    p.add(4, S.bow(rng, wb + list(range(800, 810))))
    p.cov(3, [1, 2, 4321, 4])                                 # 4321: not in the database
    p.cov(4, [2])
    ta = p.reloc(qa)
    assert ids_of(ta["scored"]) == [1]
    tb = p.reloc(qb)
    assert ids_of(tb["scored"]) == [3, 4] and set(ids_of(tb["listed"])) == {1, 2, 3, 4}
    n, m = p.ref.kf[1], p.ref.kf[2]
    assert n.mRelocScore == ta["entries"][0][0] and n.mRelocScore > 0 and f32bits(m.mRelocScore) == 0
    s = {k.mnId: si for si, k in tb["entries"]}
    acc3 = [a for (si, k), (a, _) in zip(tb["entries"], tb["acc"]) if k.mnId == 3][0]
    assert f32bits(acc3) == f32bits(F(F(F(s[3] + n.mRelocScore) + F(0)) + s[4]))       # stale + fresh 0 + scored, absent skipped
    # a loop query in between leaves the stale scores alone
    p.loop(qa, [], 0.0)
    p.reloc(qb)


def test_reloc_erase_and_readd(pkg):
    rng = np.random.default_rng(29)
    p = Pair(pkg, 2000)
    wa, wb = list(range(0, 40, 2)), list(range(1000, 1040, 2))
    qa, qb = S.bow(rng, wa), S.bow(rng, wb)
    v1 = S.bow(rng, wa[:18] + [1000] + list(range(500, 520)))
    p.add(1, v1)
    p.add(2, S.bow(rng, [1000] + wb[1:] + list(range(700, 730))))
    p.add(3, S.bow(rng, [1000] + wb[2:] + list(range(800, 810))))
    p.cov(2, [1, 3]); p.cov(1, [2]); p.cov(3, [1])
    p.reloc(qa)                                               # scores 1: it now carries a stale score
    t = p.reloc(qb)
    assert ids_of(t["listed"]) == [1, 2, 3] and p.ref.kf[1].mRelocScore > 0 and 1 not in ids_of(t["scored"])
    p.erase(1)
    p.erase(55)                                               # absent: nothing happens
    t = p.reloc(qb)
    assert ids_of(t["listed"]) == [2, 3]                      # an erased keyframe is never listed
    p.score(qb, [2, 3])
    with pytest.raises(pkg.OrbxError) as e:
        p.db.score(*S.arrays(qb), [1])
    assert e.value.status == pkg.ORBX_ERR_ARG
    p.add(1, v1)
    t = p.reloc(qb)
    assert ids_of(t["listed"]) == [2, 3, 1]                   # re-added: at the end of word 1000's list
    assert f32bits(p.ref.kf[1].mRelocScore) == 0 and p.ref.cov[1] == []                  # stale score and covisible list gone
    assert p.db.info()["keyframes"] == 3
    p.cov(1, [2])
    p.reloc(qa); p.reloc(qb); p.loop(qb, [3], 0.0)


def test_argument_errors_on_a_handle(pkg):
    p = Pair(pkg, 100)
    L, h = p.db._L, p.db._h
    w = np.array([1, 5, 9], np.uint32); v = np.array([.2, .3, .5]); n = C.c_int(0); nh = C.c_int(0)
    ptr = lambda a: a.ctypes.data   # noqa: E731
    E = pkg.ORBX_ERR_ARG
    assert L.orbv_db_add(h, 1, ptr(w), ptr(v), 3) == 0
    assert L.orbv_db_add(h, 1, ptr(w), ptr(v), 3) == E                                          # already present
    flat, big, swapped = np.array([1, 1, 9], np.uint32), np.array([1, 5, 100], np.uint32), np.array([5, 1, 9], np.uint32)
    neg, pair13, minus1 = np.array([2, -2], np.int32), np.array([1, 3], np.int32), np.array([-1], np.int32)
    two = np.zeros(2)
    assert L.orbv_db_add(h, 2, ptr(flat), ptr(v), 3) == E                                       # not strictly ascending
    assert L.orbv_db_add(h, 2, ptr(big), ptr(v), 3) == E                                        # >= nwords
    assert L.orbv_db_add(h, -1, ptr(w), ptr(v), 3) == E
    assert L.orbv_db_add(h, pkg.DB_MAX_KF_ID + 1, ptr(w), ptr(v), 3) == pkg.ORBX_ERR_UNSUPPORTED
    assert L.orbv_db_add(h, pkg.DB_MAX_KF_ID, None, None, 0) == 0                               # n == 0 is legal, the bound itself too
    assert L.orbv_db_erase(h, -1) == E and L.orbv_db_erase(h, 50) == 0
    ids = np.arange(11, dtype=np.int32)
    assert L.orbv_db_set_covisible(h, 1, ptr(ids), 11) == E and L.orbv_db_set_covisible(h, 1, ptr(ids), 10) == 0
    assert L.orbv_db_set_covisible(h, 3, ptr(ids), 2) == E                                      # absent keyframe
    assert L.orbv_db_set_covisible(h, 1, ptr(neg), 2) == E
    assert L.orbv_db_score(h, ptr(w), ptr(v), 3, ptr(pair13), 2, ptr(two)) == E
    cand = np.zeros(4, np.int32)
    assert L.orbv_db_detect_loop(h, ptr(w), ptr(v), 3, ptr(minus1), 1, 0.0, ptr(cand), 4, C.byref(n), None, 0, None) == E
    assert L.orbv_db_detect_reloc(h, ptr(swapped), ptr(v), 3, ptr(cand), 4, C.byref(n), None, 0, None) == E
    # capacities too small: the needed counts come back
    hits = np.zeros(1, pkg.DB_HIT_DTYPE)
    assert L.orbv_db_detect_reloc(h, ptr(w), ptr(v), 3, None, 0, C.byref(n), None, 0, C.byref(nh)) == E and (n.value, nh.value) == (1, 1)
    assert L.orbv_db_add(h, 2, ptr(w), ptr(v), 3) == 0
    assert L.orbv_db_detect_reloc(h, ptr(w), ptr(v), 3, ptr(cand), 4, C.byref(n), ptr(hits), 1, C.byref(nh)) == E and nh.value == 2
    # an empty query and nothing listed: ORBX_OK, zero candidates
    assert L.orbv_db_detect_reloc(h, None, None, 0, ptr(cand), 4, C.byref(n), None, 0, C.byref(nh)) == 0 and (n.value, nh.value) == (0, 0)
    w2 = np.array([2, 3], np.uint32)
    assert L.orbv_db_detect_loop(h, ptr(w2), ptr(v), 2, None, 0, 0.0, ptr(cand), 4, C.byref(n), None, 0, C.byref(nh)) == 0 and (n.value, nh.value) == (0, 0)
    assert p.db.info()["keyframes"] == 3 and p.db.info()["entries"] == 6


def test_pool_regrows_and_clear(pkg):
    rng = np.random.default_rng(30)
    p = Pair(pkg, 500, initial_entries=64)
    kfs, cov = S.crowd(rng, 500, 300, 20)
    q = S.random_bow(rng, 500, 80)
    ids = sorted(kfs)
    for i in ids[:2]:
        p.add(i, kfs[i])
    assert p.db.info()["pool_entries"] == 64
    t = p.reloc(q)
    for i in ids[2:]:
        p.add(i, kfs[i])
    for i, c in cov.items():
        p.cov(i, c)
    info = p.db.info()
    assert info["keyframes"] == 300 and info["entries"] == 6000 and info["pool_entries"] >= 6000 and info["device_bytes"] >= 6000 * 12
    t = p.reloc(q)
    assert len(t["listed"]) > 250
    p.loop(q, ids[:7], 0.02)
    p.score(q, ids[::7])
    # clear, then reuse: the old keyframes are gone, ids can be taken again
    p.clear()
    assert p.db.info()["keyframes"] == 0 and p.db.info()["entries"] == 0
    assert len(p.db.detect_relocalization_candidates(*S.arrays(q))) == 0
    for k, i in enumerate(ids[:40]):
        p.add(i, kfs[ids[-1 - k]])
    p.cov(ids[0], ids[1:9])
    t = p.reloc(q)
    assert 30 < len(t["listed"]) <= 40
    p.loop(q, [], 0.0)


def test_two_handles_from_two_threads(pkg):
    rng = np.random.default_rng(31)
    pairs, queries = [], []
    for k in range(2):
        p = Pair(pkg, 400)
        kfs, cov = S.crowd(rng, 400, 60 + 10 * k, 30)
        p.fill(kfs, cov)
        pairs.append(p); queries.append([S.random_bow(rng, 400, 50) for _ in range(6)])
    errors = []

    def work(p, qs):
        try:
            for q in qs:
                p.reloc(q); p.loop(q, [3, 4], 0.01)
        except BaseException as e:   # noqa: B902
            errors.append(e)
    th = [threading.Thread(target=work, args=(p, qs)) for p, qs in zip(pairs, queries)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors


def test_shared_handle_query_while_adding(pkg):
    """one thread repeats a loop query while another adds keyframes sharing no word with it: every repetition equals the first"""
    rng = np.random.default_rng(32)
    db = pkg.KeyFrameDatabase(2000, initial_entries=256)
    kfs, cov = S.crowd(rng, 400, 50, 30)
    for i in kfs:
        db.add(i, *S.arrays(kfs[i]))
    for i, c in cov.items():
        db.set_covisible(i, c)
    qw, qv = S.arrays(S.random_bow(rng, 400, 50))
    first_c, first_h = db.detect_loop_candidates(qw, qv, [2, 5], 0.01, hits=True)
    assert len(first_h) > 30 and len(first_c) >= 1
    errors, results = [], []

    def adder():
        try:
            for k in range(120):
                w = 400 + np.sort(np.random.default_rng(k).choice(1600, 25, replace=False)).astype(np.uint32)
                db.add(1000 + k, w, np.full(25, 0.04))
        except BaseException as e:   # noqa: B902
            errors.append(e)

    def asker():
        try:
            for _ in range(40):
                results.append(db.detect_loop_candidates(qw, qv, [2, 5], 0.01, hits=True))
        except BaseException as e:   # noqa: B902
            errors.append(e)
    th = [threading.Thread(target=adder), threading.Thread(target=asker)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errors, errors
    assert db.info()["keyframes"] == 170 and db.info()["pool_entries"] >= 50 * 30 + 120 * 25
    for c, h in results:
        assert (c == first_c).all() and h.tobytes() == first_h.tobytes()


def test_hand_worked_database_on_the_gpu(pkg):
    p = Pair(pkg, S.HAND_NWORDS)
    p.fill(S.HAND_KFS, S.HAND_COV)
    assert list(p.db.detect_relocalization_candidates(*S.arrays(S.HAND_QUERY))) == [10]
    p.reloc(S.HAND_QUERY); p.loop(S.HAND_QUERY, [], 0.4); p.loop(S.HAND_QUERY, [], 0.375); p.loop(S.HAND_QUERY, [10], 0.3)
    assert list(p.score(S.HAND_QUERY, [12, 10, 11])) == [0.25, 0.5, 0.375]
