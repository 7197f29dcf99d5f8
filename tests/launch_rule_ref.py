"""The launch rule of an extraction call, restated in plain Python for tests/test_launch_plan_cpu.py.

Written from launch_chunk of csrc/orbx_extract.hip as it stood BEFORE the rule moved into plan_chunk (csrc/orbx_plan.h): one
expression here per expression there, in that function's order, with the repetitions it had (the strip rule and the 1024-thread rule
were each written out more than once; they are evaluated more than once here and asserted equal).  It does not read orbx_plan.h.
Inputs: the PlanInput fields by name (orb_slam2v2-1_amd.PLAN_INPUT_FIELDS), `ncells` per level, `opt` = {key: value} or a list of 32.
Output: the ChunkPlan as a flat tuple of ints, FIELDS then nslice[16] (as_dict names them).  Where launch_chunk computed a value only on one path (the
compaction decision inside the strip branch, the multi-workgroup mask inside the k_octree_pyr branch) the value is 0 on the others.
"""
HIST_IMAGES = 4          # ORBX_HIST_IMAGES
SPARSE_PER_CELL = 16     # ORBX_SPARSE_PER_CELL
MAX_LEVELS = 16
OCT_EXACT, OCT_BIG, OCT_EARLY, OCT_SPLIT, OCT_SINGLE = range(5)
HINT_NONE, HINT_OCT_SRC, HINT_GATHER = range(3)
FIELDS = ["usePyr", "strips", "stripLevels", "fastCells", "es", "histOct", "multiWg", "fused", "gather", "bigMask", "wideOct", "compact", "sparseForm",
          "sparsePerCell", "rowFlags", "sparseHint", "earlyLv", "aSplit", "octForm", "sweepSlices", "sweepShared", "orderKernel", "fastDoneAt",
          "fastPhase", "octPhase", "octStop", "descLdsPad"]


def chunk_count(B, prof=0, skipPyr=0, opt=None):
    """Chunks a batch of B images is cut into (chunk_count, restated the same way); chunk 0 holds B // chunks images."""
    o = opt or {}
    nch = 1 if o.get(8, 0) <= 1 else min(o[8], 4)
    nch = min(nch, B)
    if prof or skipPyr or o.get(0, 0) or o.get(1, 0) or o.get(7, 0):
        nch = 1
    return nch


def option_list(opt):
    o = [0] * 32
    for k, v in (opt or {}).items():
        o[k] = v
    return o


def plan(B, nl, totalStrips, stripLevels, octBigMask, lastChunks, prof=0, profFast=0, skipPyr=0, pfUsed=0, evPyrDone=0, dbgBlur=0,
         sliceScratch=0, fastTileStride=0, fastScoreStride=0, sparseRecent=0, ncells=(), opt=None):
    o = opt if isinstance(opt, list) else option_list(opt)
    # the ordering kernel in front of the FAST start event; the gate of a pyramid built ahead, option 10 = 3
    orderKernel = profFast and skipPyr and o[12] == 0
    fast_done = 3 if (pfUsed and not evPyrDone and o[10] == 3) else -1
    # decisions of the quad-tree stage that the FAST stage needs to know
    usePyr = o[4] != 1
    stripsWanted = totalStrips > 0 and (totalStrips * B >= 4096 if o[6] == 0 else o[6] == 3)
    histWanted = (o[23] == 0 and B <= HIST_IMAGES and lastChunks == 1 and not stripsWanted and o[0] == 0 and o[18] != 1 and
                  o[7] == 0 and o[1] == 0)
    multiWg = o[4] == 2 or (o[4] != 3 and B <= 4 and octBigMask != 0 and not histWanted)
    fused = usePyr and not multiWg and o[7] in (0, 8, 9) and o[1] == 0 and o[18] != 1
    sparsePerCell = 1 << 20 if o[16] == 2 else SPARSE_PER_CELL
    hint_oct_src = fused and o[20] != 0          # OctSrc::sparseSeen
    histOct = fused and histWanted
    wideOct = (octBigMask != 0) if o[11] == 0 else o[11] == 2
    compact, earlyLv, rowFlags = False, 0, False
    # K2
    strips = totalStrips > 0 and (totalStrips * B >= 4096 if o[6] == 0 else o[6] == 3)
    assert strips == stripsWanted
    planStripLevels = stripLevels if strips else 0
    if strips:
        rowFlags = o[16] != 1                    # spf != NULL
        compact = rowFlags and o[20] != 0 and (o[16] == 2 or bool(sparseRecent))
        ea = o[19]
        if (fused and not prof and not compact and o[19] >= 2 and o[15] < 2 and lastChunks == 1 and B >= 8 and nl > ea and
                (stripLevels & ((1 << ea) - 1)) == (1 << ea) - 1 and not dbgBlur):
            earlyLv = ea
    es = fastTileStride if (fastScoreStride == fastTileStride - 8 and o[6] != 2) else 0
    es = es if es in (44, 48, 52) else 0         # switch (es): the compiled instances, anything else the run-time-stride one
    fastCells = planStripLevels != (1 << nl) - 1
    gate = pfUsed and not evPyrDone
    if gate and o[10] == 0:
        fast_done = 0
    # K3
    hint_gather = (not fused) and o[20] != 0     # k_gather's sparseSeen argument
    aSplit = min(o[15], nl - 1) if (usePyr and not prof and lastChunks == 1 and B >= 8 and o[7] == 0 and o[1] == 0 and o[15] >= 2 and
                                    not multiWg and not dbgBlur) else 0
    if nl < 3:
        aSplit = 0
    bigMask, form, slices, shared, nslice = 0, None, False, False, [0] * MAX_LEVELS
    if usePyr:
        bigMask = 0 if not multiWg else ((1 << nl) - 1 if o[4] == 2 else octBigMask)
        nBig = bin(bigMask & ((1 << nl) - 1)).count("1")      # levels l < nl with bit l set
        wide = (octBigMask != 0) if o[11] == 0 else o[11] == 2
        assert wide == wideOct
        if nBig > 0 and o[7] == 0 and o[1] == 0:
            form = OCT_BIG
        elif earlyLv > 0:
            form = OCT_EARLY
        elif aSplit > 0:
            form = OCT_SPLIT
        else:
            form = OCT_SINGLE
            kmax = 1
            if fused and not histOct and o[26] == 1 and sliceScratch and o[7] == 0 and o[1] == 0:
                slices = True
                for l in range(nl):
                    nslice[l] = 4 if ncells[l] >= 1600 else 2 if ncells[l] >= 600 else 1
                    kmax = max(kmax, nslice[l])
            shared = kmax > 1
    else:
        wide = (octBigMask != 0) if o[11] == 0 else o[11] == 2
        assert wide == wideOct
        form = OCT_EXACT
    if gate and o[10] == 1:
        fast_done = 1
    # K4
    if gate and o[10] == 2:
        fast_done = 2
    return (usePyr, strips, planStripLevels, fastCells, es, histOct, multiWg, fused, not fused, bigMask, wideOct, compact, o[20], sparsePerCell,
        rowFlags, HINT_OCT_SRC if hint_oct_src else HINT_GATHER if hint_gather else HINT_NONE, earlyLv, aSplit, form, slices, shared,
        orderKernel, fast_done, o[0], o[1], o[7], o[21] * 1024) + tuple(nslice)      # (flags as bools: True == 1)


def as_dict(t):
    d = {k: int(v) for k, v in zip(FIELDS, t)}
    d["nslice"] = tuple(t[len(FIELDS):])
    return d
