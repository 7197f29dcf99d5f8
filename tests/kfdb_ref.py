"""Restatement of ORB_SLAM2::KeyFrameDatabase (src/KeyFrameDatabase.cc:31-309) and DBoW2's L1Scoring::score
(Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68) in plain Python, written from the reference's text: real inverted lists per
word, keyframe objects with the reference's stamp members, the two Detect* functions line by line.  numpy.float32 for every
float step, Python floats for the doubles.  A BoW vector is a list of (word id, value) pairs in ascending id (the iteration
order of the reference's std::map).

What is a hypothesis, not the reference's text: mRelocScore starts at float32(0) (src/KeyFrame.cc:35 leaves it uninitialised).
The caller passes query ids that are never repeated and never 0, as DetectLoop and Relocalization do."""
import bisect

import numpy as np

F = np.float32


def lower_bound(v, pos, wid):
    """std::map::lower_bound on the sorted pair list: first position whose id is >= wid"""
    return bisect.bisect_left(v, (wid, -np.inf))


def score(v1, v2):
    """L1Scoring::score, ScoringObject.cpp:23-68, with the lower_bound skips as written"""
    i, j = 0, 0
    s = 0.0
    while i != len(v1) and j != len(v2):
        vi, wi = v1[i][1], v2[j][1]
        if v1[i][0] == v2[j][0]:
            s += abs(vi - wi) - abs(vi) - abs(wi)
            i += 1
            j += 1
        elif v1[i][0] < v2[j][0]:
            i = lower_bound(v1, i, v2[j][0])
        else:
            j = lower_bound(v2, j, v1[i][0])
    s = -s / 2.0
    return s


class KeyFrame:
    def __init__(self, mnId, bow):
        self.mnId = mnId
        self.mBowVec = list(bow)
        self.mnLoopQuery = 0
        self.mnLoopWords = 0
        self.mLoopScore = F(0)
        self.mnRelocQuery = 0
        self.mnRelocWords = 0
        self.mRelocScore = F(0)
        self.covisible = []          # GetBestCovisibilityKeyFrames(10): KeyFrame objects, the caller's graph

    def __repr__(self):
        return "KF%d" % self.mnId


class KeyFrameDatabase:
    def __init__(self, nwords):
        self.nwords = nwords
        self.mvInvertedFile = [[] for _ in range(nwords)]

    def add(self, pKF):                                              # :40-46
        for wid, _ in pKF.mBowVec:
            self.mvInvertedFile[wid].append(pKF)

    def erase(self, pKF):                                            # :48-67
        for wid, _ in pKF.mBowVec:
            lKFs = self.mvInvertedFile[wid]
            for k, other in enumerate(lKFs):
                if other is pKF:
                    del lKFs[k]
                    break

    def clear(self):                                                 # :69-73
        self.mvInvertedFile = [[] for _ in range(self.nwords)]

    def DetectLoopCandidates(self, qid, qbow, connected, minScore, trace=None):   # :76-197
        minScore = F(minScore)
        spConnectedKeyFrames = set(connected)                        # KeyFrame objects
        lKFsSharingWords = []
        for wid, _ in qbow:
            for pKFi in self.mvInvertedFile[wid]:
                if pKFi.mnLoopQuery != qid:
                    pKFi.mnLoopWords = 0
                    if pKFi not in spConnectedKeyFrames:
                        pKFi.mnLoopQuery = qid
                        lKFsSharingWords.append(pKFi)
                pKFi.mnLoopWords += 1
        if trace is not None:
            trace.update(listed=list(lKFsSharingWords), scored=[], entries=[], acc=[], maxCommonWords=0, minCommonWords=0)
        if not lKFsSharingWords:
            return []
        lScoreAndMatch = []
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > maxCommonWords:
                maxCommonWords = pKFi.mnLoopWords
        minCommonWords = int(F(maxCommonWords) * F(0.8))
        for pKFi in lKFsSharingWords:
            if pKFi.mnLoopWords > minCommonWords:
                si = F(score(qbow, pKFi.mBowVec))
                pKFi.mLoopScore = si
                if trace is not None:
                    trace["scored"].append(pKFi)
                if si >= minScore:
                    lScoreAndMatch.append((si, pKFi))
        if trace is not None:
            trace.update(maxCommonWords=maxCommonWords, minCommonWords=minCommonWords, entries=list(lScoreAndMatch))
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = minScore
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = si
            pBestKF = pKFi
            for pKF2 in pKFi.covisible:
                if pKF2.mnLoopQuery == qid and pKF2.mnLoopWords > minCommonWords:
                    accScore = F(accScore + pKF2.mLoopScore)
                    if pKF2.mLoopScore > bestScore:
                        pBestKF = pKF2
                        bestScore = pKF2.mLoopScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F(F(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpLoopCandidates = []
        for acc, pKFi in lAccScoreAndMatch:
            if acc > minScoreToRetain:
                if pKFi not in spAlreadyAddedKF:
                    vpLoopCandidates.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
        if trace is not None:
            trace.update(acc=list(lAccScoreAndMatch), bestAccScore=bestAccScore, minScoreToRetain=minScoreToRetain)
        return vpLoopCandidates

    def DetectRelocalizationCandidates(self, qid, qbow, trace=None):               # :199-309
        lKFsSharingWords = []
        for wid, _ in qbow:
            for pKFi in self.mvInvertedFile[wid]:
                if pKFi.mnRelocQuery != qid:
                    pKFi.mnRelocWords = 0
                    pKFi.mnRelocQuery = qid
                    lKFsSharingWords.append(pKFi)
                pKFi.mnRelocWords += 1
        if trace is not None:
            trace.update(listed=list(lKFsSharingWords), scored=[], entries=[], acc=[], maxCommonWords=0, minCommonWords=0)
        if not lKFsSharingWords:
            return []
        maxCommonWords = 0
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > maxCommonWords:
                maxCommonWords = pKFi.mnRelocWords
        minCommonWords = int(F(maxCommonWords) * F(0.8))
        lScoreAndMatch = []
        for pKFi in lKFsSharingWords:
            if pKFi.mnRelocWords > minCommonWords:
                si = F(score(qbow, pKFi.mBowVec))
                pKFi.mRelocScore = si
                lScoreAndMatch.append((si, pKFi))
                if trace is not None:
                    trace["scored"].append(pKFi)
        if trace is not None:
            trace.update(maxCommonWords=maxCommonWords, minCommonWords=minCommonWords, entries=list(lScoreAndMatch))
        if not lScoreAndMatch:
            return []
        lAccScoreAndMatch = []
        bestAccScore = F(0)
        for si, pKFi in lScoreAndMatch:
            bestScore = si
            accScore = bestScore
            pBestKF = pKFi
            for pKF2 in pKFi.covisible:
                if pKF2.mnRelocQuery != qid:
                    continue
                accScore = F(accScore + pKF2.mRelocScore)
                if pKF2.mRelocScore > bestScore:
                    pBestKF = pKF2
                    bestScore = pKF2.mRelocScore
            lAccScoreAndMatch.append((accScore, pBestKF))
            if accScore > bestAccScore:
                bestAccScore = accScore
        minScoreToRetain = F(F(0.75) * bestAccScore)
        spAlreadyAddedKF = set()
        vpRelocCandidates = []
        for si, pKFi in lAccScoreAndMatch:
            if si > minScoreToRetain:
                if pKFi not in spAlreadyAddedKF:
                    vpRelocCandidates.append(pKFi)
                    spAlreadyAddedKF.add(pKFi)
        if trace is not None:
            trace.update(acc=list(lAccScoreAndMatch), bestAccScore=bestAccScore, minScoreToRetain=minScoreToRetain)
        return vpRelocCandidates


class Session:
    """The reference database driven by ids, as the library's interface is: keeps KeyFrame objects per id (a re-added id is a
    fresh KeyFrame, as a new keyframe is in the reference), covisible lists as ids resolved at query time (an id that is not in
    the database is no KeyFrame the database could have stamped: skipped), and hands out query ids 1, 2, 3, ..."""

    def __init__(self, nwords):
        self.db = KeyFrameDatabase(nwords)
        self.kf = {}
        self.cov = {}
        self.qid = 0

    def add(self, kf_id, bow):
        assert kf_id not in self.kf
        self.kf[kf_id] = KeyFrame(kf_id, bow)
        self.cov[kf_id] = []
        self.db.add(self.kf[kf_id])

    def erase(self, kf_id):
        if kf_id in self.kf:
            self.db.erase(self.kf.pop(kf_id))
            del self.cov[kf_id]

    def clear(self):
        self.db.clear()
        self.kf.clear()
        self.cov.clear()

    def set_covisible(self, kf_id, ids):
        assert kf_id in self.kf and len(ids) <= 10
        self.cov[kf_id] = list(ids)

    def _bind(self):
        for k, pKF in self.kf.items():
            pKF.covisible = [self.kf[i] for i in self.cov[k] if i in self.kf]

    def score(self, qbow, ids):
        return [score(qbow, self.kf[i].mBowVec) for i in ids]

    def _hits(self, t, words, mscore):
        """the library's orbv_db_hit_t records from a trace: (kf_id, words, flags, score, acc_score, best_kf) per listed keyframe"""
        scored = set(id(k) for k in t["scored"])
        acc = {id(e[1]): a for e, a in zip(t["entries"], t["acc"])}
        out = []
        for k in t["listed"]:
            fl = (1 if id(k) in scored else 0) | (2 if id(k) in acc else 0)
            a = acc.get(id(k))
            out.append((k.mnId, getattr(k, words), fl, mscore(k, fl), a[0] if a else F(0), a[1].mnId if a else -1))
        return out

    def detect_loop(self, qbow, connected, min_score):
        self._bind()
        self.qid += 1
        t = {}
        cand = self.db.DetectLoopCandidates(self.qid, qbow, [self.kf[i] for i in connected if i in self.kf], min_score, t)
        return [k.mnId for k in cand], self._hits(t, "mnLoopWords", lambda k, fl: k.mLoopScore if fl & 1 else F(0)), t

    def detect_reloc(self, qbow):
        self._bind()
        self.qid += 1
        t = {}
        cand = self.db.DetectRelocalizationCandidates(self.qid, qbow, t)
        return [k.mnId for k in cand], self._hits(t, "mnRelocWords", lambda k, fl: k.mRelocScore), t
