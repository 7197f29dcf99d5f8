"""Seeded builders of BoW vectors and small keyframe databases for the keyframe-database tests (tests/test_kfdb_*.py).
A BoW vector is a list of (word id, value) pairs in ascending id.  Values are positive random doubles normalised by a
sequential L1 sum (BowVector::normalize), so no partial sum of a score is exact in binary."""
import numpy as np


def values(rng, n):
    x = [float(v) for v in rng.uniform(0.05, 1.0, n)]
    norm = 0.0
    for v in x:
        norm += abs(v)
    return [v / norm for v in x]


def bow(rng, words):
    words = sorted(set(int(w) for w in words))
    return list(zip(words, values(rng, len(words))))


def random_bow(rng, nwords, n):
    return bow(rng, rng.choice(nwords, n, replace=False)) if n else []


def arrays(v):
    return np.array([w for w, _ in v], np.uint32), np.array([x for _, x in v], np.float64)


def overlapping_query(rng, nwords, kfs, n):
    """n words: about half drawn from the words the keyframe vectors hold, the rest anywhere"""
    held = sorted(set(w for v in kfs for w, _ in v))
    take = min(len(held), max(1, n // 2))
    words = set(int(w) for w in rng.choice(held, take, replace=False))
    rest = [w for w in rng.permutation(nwords) if int(w) not in words]
    words.update(int(w) for w in rest[:n - len(words)])
    assert len(words) == n
    return bow(rng, words)


def crowd(rng, nwords, nkf, kf_len, first_id=1, absent_id=None):
    """nkf keyframes of kf_len words each over a small vocabulary (so that all overlap), ids first_id .., and for each a
    covisible list of up to 10 other ids (absent_id, when given, is sprinkled in: an id the database does not hold)"""
    ids = list(range(first_id, first_id + nkf))
    kfs = {i: random_bow(rng, nwords, kf_len) for i in ids}
    cov = {}
    for i in ids:
        others = [j for j in ids if j != i]
        k = int(rng.integers(0, min(10, len(others)) + 1))
        c = [int(j) for j in rng.choice(others, k, replace=False)] if k else []
        if absent_id is not None and c and rng.random() < 0.3:
            c[int(rng.integers(0, len(c)))] = absent_id
        cov[i] = c
    return kfs, cov


def with_common(rng, qwords, ncommon, private, nprivate):
    """a keyframe vector holding exactly ncommon of the query's words (the first ncommon) and nprivate words of `private`"""
    return bow(rng, list(qwords[:ncommon]) + list(private[:nprivate]))


# A database worked by hand (tests/test_kfdb_cpu.py writes out what its queries must give).  Values are binary fractions, so
# every step is exact.  Keyframes are added in id order.
HAND_NWORDS = 16
HAND_QUERY = [(2, 0.25), (4, 0.25), (6, 0.25), (8, 0.25)]
HAND_KFS = {
    10: [(4, 0.25), (6, 0.5), (9, 0.25)],     # common 4, 6: (0 - .25 - .25) + (.25 - .25 - .5) = -1.0  -> score 0.5
    11: [(2, 0.125), (3, 0.25), (8, 0.625)],  # common 2, 8: (.125 - .25 - .125) + (.375 - .25 - .625) = -0.75 -> score 0.375
    12: [(1, 0.5), (8, 0.5)],                 # common 8: one word
}
HAND_COV = {10: [12], 11: [10, 12], 12: []}
