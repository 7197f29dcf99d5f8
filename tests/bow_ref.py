"""Plain numpy restatement of the DBoW2 descent and the BoW-guided matchers, written from the reference's text
(Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1230-1271, src/ORBmatcher.cc:140-157, 159-288, 522-655, 657-825,
1603-1644), NOT from oracle/orb_oracle_bow.c: tests/test_bow_cpu.py holds the C oracle to this file, so the GPU
tests of tests/test_bow_gpu.py compare against a restatement that two independent texts agree on.

Per-query loops, np.float32 where the reference has `float` (one rounding per operation, no contraction),
Python ints for distances.  Each matcher also returns a `stats` dict that says which branches of the wave-per-node
kernels (candidate p -> lane p % 64, bit p / 64 of `taken`) a case reaches:
    hi          accepted matches whose winning list position is >= 64
    same_lane   accepted matches whose runner-up position p2 has p2 % 64 == p1 % 64
    other_lane  accepted matches whose runner-up sits in another lane
    ties        accepted matches with d1 == d2
    ties_across accepted ties whose tied pair straddles two lanes (the lower position must win)
    taken_hi    candidates skipped as already taken at a position >= 64
    accepted    matches before the rotation filter; `unfiltered` is match_q at that point, `histogram` the 30 bins
search_for_triangulation reports hi, taken_hi, accepted and
    shared_last_hi  accepted matches at a position >= 64 whose minimum distance is shared by several passing
                    candidates (the LAST one wins)
"""
import numpy as np

F32 = np.float32
HISTO_LENGTH = 30
_POP8 = np.array([bin(i).count("1") for i in range(256)], np.int64)


def ham(a, B):
    """FORB::distance / ORBmatcher::DescriptorDistance of one 32-byte descriptor against rows of B."""
    x = np.bitwise_xor(np.asarray(a, np.uint8)[None, :], np.asarray(B, np.uint8).reshape(-1, 32))
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(x.view(np.uint64)).sum(1).astype(np.int64)
    return _POP8[x].sum(1)


def children(voc):
    """node -> array of its children in id order (loadFromTextFile :1351-1436 appends them as they are read)."""
    if "_children" not in voc:
        par = np.asarray(voc["parent"], np.int64)
        order = np.argsort(par[1:], kind="stable") + 1
        cnt = np.bincount(par[1:], minlength=len(par))
        start = np.concatenate([[0], np.cumsum(cnt)])
        voc["_children"] = [order[start[i]:start[i + 1]] for i in range(len(par))]
    return voc["_children"]


def path(voc, feature):
    """The do-while of :1245-1267: the nodes chosen at levels 1, 2, ... down to a childless node, and per step
    (chosen child position, positions that share the minimum distance)."""
    ch, desc = children(voc), voc["desc"]
    nodes, steps, final_id = [], [], 0
    while True:
        c = ch[final_id]
        d = ham(feature, desc[c])
        best = 0
        for j in range(1, len(c)):                      # d < best_d: the first minimum stays
            if d[j] < d[best]:
                best = j
        final_id = int(c[best])
        nodes.append(final_id)
        steps.append((best, np.flatnonzero(d == d[best])))
        if len(ch[final_id]) == 0:                       # Node::isLeaf()
            return nodes, steps


def descend(voc, feature, levelsup, nodes=None):
    """-> (leaf, nid).  nid is the node on the path at level L - levelsup, 0 (the root) when that level is <= 0,
    and None when the path ends above that level: the reference leaves *nid unset there (callers pass an
    initialised 0); the library's contract is 0."""
    if nodes is None:
        nodes, _ = path(voc, feature)
    nid_level = int(voc["L"]) - int(levelsup)
    if nid_level <= 0:
        nid = 0
    elif nid_level <= len(nodes):
        nid = nodes[nid_level - 1]
    else:
        nid = None
    return nodes[-1], nid


def word_of(voc, leaf):
    """-> (word_id, weight) of the node a descent ends in: words are the nodes flagged nIsLeaf, numbered in id
    order (:1421-1428); a childless node without the flag keeps Node()'s word_id 0 and weight 0 (:313-318)."""
    if "_word" not in voc:
        flag = np.asarray(voc["is_leaf"], np.int64).copy()
        flag[0] = 0                                      # the root is not in the file
        voc["_word"] = np.cumsum(flag) - 1
    if leaf > 0 and voc["is_leaf"][leaf]:
        return int(voc["_word"][leaf]), float(voc["weight"][leaf])
    return 0, 0.0


def three_maxima(h):
    """ORBmatcher::ComputeThreeMaxima (:1603-1644) on the bin sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(int(x) for x in h):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    tenth = F32(0.1) * F32(max1)                         # 0.1f*(float)max1, compared with an int: exact in double
    if max2 < float(tenth):
        ind2 = ind3 = -1
    elif max3 < float(tenth):
        ind3 = -1
    return ind1, ind2, ind3


def rotation_bin(a1, a2):
    """float rot = a1 - a2; if(rot<0.0) rot+=360.0f; int bin = round(rot*factor); if(bin==HISTO_LENGTH) bin=0;"""
    rot = F32(a1) - F32(a2)
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    x = F32(rot * (F32(1.0) / F32(HISTO_LENGTH)))
    r = np.floor(x)
    b = int(r) + (1 if x - r >= F32(0.5) else 0)         # round(): halves away from zero (x >= 0 here, -0.0 -> 0)
    return 0 if b == HISTO_LENGTH else b


def _rotation_filter(match_q, nmatches, aq, ac, order):
    """The rotHist bookkeeping and the tail loop (:267-285): matches outside the three largest bins go."""
    bins = {iq: rotation_bin(aq[iq], ac[match_q[iq]]) for iq in order}
    h = np.zeros(HISTO_LENGTH, np.int64)
    for b in bins.values():
        assert 0 <= b < HISTO_LENGTH
        h[b] += 1
    keep = three_maxima(h)
    for iq, b in bins.items():
        if b not in keep:
            match_q[iq] = -1
            nmatches -= 1
    return nmatches, h


def search_by_bow(qd, qa, qv, cd, ca, cv, nqs, qit, ncs, cit, max_dist, nnratio, check_orientation=True):
    """SearchByBoW on the intersected node lists -> (nmatches, match_q, stats).  cv None: the KeyFrame-Frame
    overload (every candidate; max_dist = TH_LOW for its `<=`); cv given: the KeyFrame-KeyFrame overload
    (candidates need a good map point; max_dist = TH_LOW - 1 for its `<`)."""
    nq, nc = len(qa), len(ca)
    match_q = np.full(nq, -1, np.int32)
    taken = np.zeros(nc, bool)                            # vpMapPointMatches[realIdxF] / vbMatched2[idx2]
    st = dict(hi=0, same_lane=0, other_lane=0, ties=0, ties_across=0, taken_hi=0, accepted=0)
    order = []
    ratio = F32(nnratio)
    for j in range(len(nqs) - 1):
        C = np.asarray(cit[ncs[j]:ncs[j + 1]], np.int64)
        for iq in (int(x) for x in qit[nqs[j]:nqs[j + 1]]):
            if not qv[iq]:
                continue
            was_taken = taken[C]
            st["taken_hi"] += int(was_taken[64:].sum())
            ok = ~was_taken if cv is None else (~was_taken) & (np.asarray(cv)[C] != 0)
            pos = np.flatnonzero(ok)
            best1, best2, p1, p2 = 256, 256, -1, -1
            if len(pos):
                d = ham(qd[iq], cd[C[pos]]).tolist()
                for t, dist in enumerate(d):              # the if / else-if of :216-225 in list order
                    if dist < best1:
                        best2, p2 = best1, p1
                        best1, p1 = dist, int(pos[t])
                    elif dist < best2:
                        best2, p2 = dist, int(pos[t])
            if p1 >= 0 and best1 <= max_dist and F32(best1) < ratio * F32(best2):   # (p1 < 0: bestIdx stays -1)
                ic = int(C[p1])
                match_q[iq] = ic
                taken[ic] = True
                order.append(iq)
                st["accepted"] += 1
                st["hi"] += p1 >= 64
                if p2 >= 0:
                    same = p2 % 64 == p1 % 64
                    st["same_lane"] += same
                    st["other_lane"] += not same
                    if best1 == best2:
                        assert p1 < p2
                        st["ties"] += 1
                        st["ties_across"] += not same
    nmatches = len(order)
    st["unfiltered"] = match_q.copy()                     # what check_orientation = False returns
    if check_orientation:
        nmatches, st["histogram"] = _rotation_filter(match_q, nmatches, qa, ca, order)
    return nmatches, match_q, st


def check_dist_epipolar_line(kp1, kp2, F12, sigma2):
    """ORBmatcher::CheckDistEpipolarLine (:140-157)."""
    F = np.asarray(F12, F32).reshape(3, 3)
    x1, y1, x2, y2 = F32(kp1["x"]), F32(kp1["y"]), F32(kp2["x"]), F32(kp2["y"])
    a = x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0]
    b = x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1]
    c = x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2]
    num = a * x2 + b * y2 + c
    den = a * a + b * b
    if den == 0:
        return False
    with np.errstate(over="ignore", invalid="ignore"):
        dsqr = num * num / den
    return bool(float(dsqr) < 3.84 * float(F32(sigma2[int(kp2["octave"])])))


def search_for_triangulation(k1, qd, qf, k2, cd, cf, nqs, qit, ncs, cit, F12, ex, ey, sf, sigma2, max_dist=50,
                             check_orientation=True):
    """SearchForTriangulation on the intersected node lists -> (nmatches, match_q, stats).  flags: bit 0 usable
    (no map point, bOnlyStereo rule applied by the caller), bit 1 mvuRight >= 0."""
    nq, nc = len(k1), len(k2)
    match_q = np.full(nq, -1, np.int32)
    matched2 = np.zeros(nc, bool)
    st = dict(hi=0, taken_hi=0, accepted=0, shared_last_hi=0)
    order = []
    ex, ey = F32(ex), F32(ey)
    sf = np.asarray(sf, F32)
    with np.errstate(under="ignore"):
        for j in range(len(nqs) - 1):
            C = np.asarray(cit[ncs[j]:ncs[j + 1]], np.int64)
            for idx1 in (int(x) for x in qit[nqs[j]:nqs[j + 1]]):
                if not qf[idx1] & 1:
                    continue
                stereo1 = bool(qf[idx1] & 2)
                was = matched2[C]
                st["taken_hi"] += int(was[64:].sum())
                pos = np.flatnonzero(~was & ((np.asarray(cf)[C] & 1) != 0))
                best_dist, best_p, shared = int(max_dist), -1, 0
                if len(pos):
                    d = ham(qd[idx1], cd[C[pos]])
                    for t in np.flatnonzero(d <= max_dist):   # dist>TH_LOW: continue (the rest in list order)
                        dist, idx2 = int(d[t]), int(C[pos[t]])
                        if dist > best_dist:
                            continue
                        kp2 = k2[idx2]
                        if not stereo1 and not cf[idx2] & 2:
                            distex, distey = ex - F32(kp2["x"]), ey - F32(kp2["y"])
                            if distex * distex + distey * distey < F32(100) * sf[int(kp2["octave"])]:
                                continue
                        if check_dist_epipolar_line(k1[idx1], kp2, F12, sigma2):
                            shared = shared + 1 if (best_p >= 0 and dist == best_dist) else 1
                            best_p, best_dist = int(pos[t]), dist
                if best_p >= 0:
                    match_q[idx1] = C[best_p]
                    matched2[C[best_p]] = True
                    order.append(idx1)
                    st["accepted"] += 1
                    st["hi"] += best_p >= 64
                    st["shared_last_hi"] += best_p >= 64 and shared > 1
    nmatches = len(order)
    st["unfiltered"] = match_q.copy()
    if check_orientation:
        nmatches, st["histogram"] = _rotation_filter(match_q, nmatches, k1["angle"], k2["angle"], order)
    return nmatches, match_q, st
