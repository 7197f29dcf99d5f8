// orbx_plan.h — the launch rule of an extraction call: which kernels one chunk of a batch runs, in which arrangement.
// plan_chunk is plain C++ over integers (no HIP call, no handle): launch_chunk (orbx_extract.hip) builds a PlanInput, gets a ChunkPlan
// and only executes it; every decision is taken ONCE here and the constraints the kernels rely on are checked before anything is
// launched.  Included by orbx_internal.h (the handle keeps its last plan).  Both structs are int32 only: the developer build's
// orbx_debug_plan_chunk / orbx_debug_last_plan (include/orbx_dev.h) hand them out as flat arrays in exactly this field order.
#pragma once
#include <algorithm>

// a level whose last call kept fewer FAST candidates per 30-px cell than this is "corner-sparse" (the benchmark's dense frames: ~60;
// smooth natural scenes: 2-4)
#define ORBX_SPARSE_PER_CELL 16

struct PlanInput {   // everything the rule reads
    int32_t B, nl;                                     // images of the chunk, pyramid levels
    int32_t totalStrips, stripLevels, octBigMask;      // plan geometry: strips per image, levels of k_fast_strips, levels with >= 600 FAST cells
    int32_t lastChunks;                                // chunks the call was cut into (chunk_count)
    int32_t prof, profFast, skipPyr, pfUsed;           // stage events of every stage / of the FAST stage, pyramid built ahead, prefetch in use
    int32_t evPyrDone, dbgBlur, sliceScratch;          // a pyramid-done event was passed, d_dbgBlur is set, d_octPartBest exists
    int32_t fastTileStride, fastScoreStride;
    int32_t sparseRecent;                              // the handle met a corner-sparse level within its last 16 calls (host-mapped word, read by the caller)
    int32_t ncells[ORBX_MAX_LEVELS];                   // FAST cells per level
    int32_t opt[ORBX_NUM_OPTIONS];                     // orbx_set_option
};
enum { ORBX_OCT_EXACT = 0, ORBX_OCT_BIG = 1, ORBX_OCT_EARLY = 2, ORBX_OCT_SPLIT = 3, ORBX_OCT_SINGLE = 4 };   // ChunkPlan::octForm
enum { ORBX_HINT_NONE = 0, ORBX_HINT_OCT_SRC = 1, ORBX_HINT_GATHER = 2 };                                     // ChunkPlan::sparseHint
enum { ORBX_FASTDONE_NEVER = -1, ORBX_FASTDONE_BEHIND_FAST = 0, ORBX_FASTDONE_BEHIND_OCT = 1, ORBX_FASTDONE_BEHIND_DESC = 2,
       ORBX_FASTDONE_WITH_FAST = 3 };                                                                         // ChunkPlan::fastDoneAt (= ORBX_OPT_PREFETCH_GATE)
struct ChunkPlan {   // everything the rule decides
    int32_t usePyr;                        // the quad-tree by k_octree_pyr (0: the exact form alone, ORBX_OPT_OCTREE_FORM = 1)
    int32_t strips, stripLevels;           // k_fast_strips takes part; the levels it does (bit l)
    int32_t fastCells, es;                 // k_fast_cells takes part (some level is not a strip level); its compile-time tile stride (44 / 48 / 52, 0 = run-time)
    int32_t histOct;                       // the FAST stage histograms its emissions and k_octree_pyr loads the histogram
    int32_t multiWg, fused, gather;        // multi-workgroup quad-tree; k_octree_pyr reads the FAST cell lists in place; k_gather runs (= !fused)
    int32_t bigMask, wideOct;              // levels shared by OCT_BIG_K workgroups; the 1024-thread quad-tree instances
    int32_t compact, sparseForm;           // a compaction kernel takes the corner-sparse (image, level)s; its form (ORBX_OPT_SPARSE_FORM)
    int32_t sparsePerCell, rowFlags;       // the density below which a level is flagged sparse; k_fast_strips gets the flags
    int32_t sparseHint;                    // who stores the "sparse level seen" hint: nobody, k_octree_pyr (OctSrc) or k_gather
    int32_t earlyLv, aSplit;               // > 0: early quad-tree of the levels [0, earlyLv) / split call at level aSplit
    int32_t octForm;                       // the quad-tree form launched (ORBX_OCT_*)
    int32_t sweepSlices, sweepShared;      // single form: OctSrc carries slice counts + scratch; some level has more than one slice (linear grid)
    int32_t orderKernel;                   // k_nop in front of the FAST stage's start event
    int32_t fastDoneAt;                    // where evFastDone is recorded (ORBX_FASTDONE_*)
    int32_t fastPhase, octPhase, octStop;  // pass-through kernel arguments: options 0, 1, 7 (phase stops / time stamps of the developer build)
    int32_t descLdsPad;                    // bytes of unused dynamic LDS per k_describe workgroup
    int32_t nslice[ORBX_MAX_LEVELS];       // sweepSlices: workgroups that share the key sweep of level l
};
#define ORBX_PLAN_INPUT_INTS (16 + ORBX_MAX_LEVELS + ORBX_NUM_OPTIONS)
#define ORBX_CHUNK_PLAN_INTS (27 + ORBX_MAX_LEVELS)
static_assert(sizeof(PlanInput) == 4 * ORBX_PLAN_INPUT_INTS && sizeof(ChunkPlan) == 4 * ORBX_CHUNK_PLAN_INTS, "flat int32 layouts of include/orbx_dev.h");

// Chunks a batch of B images is cut into (ORBX_OPT_CHUNKS; default ONE).  The one rule for launch_pipeline and orbx_fast_kernels.
static inline int chunk_count(const int *opt, int B, bool prof, bool skipPyr) {
    int nch = opt[8] <= 1 ? 1 : std::min(opt[8], ORBX_MAX_CHUNKS);
    nch = std::min(nch, B);
    if (prof || skipPyr || opt[0] || opt[1] || opt[7]) nch = 1;
    return nch;
}

static inline bool plan_implies(bool a, bool b) { return !a || b; }
#define ORBX_PLAN_NEEDS(COND)                                                                               \
    do {                                                                                                    \
        if (!(COND)) { orbx_set_error("plan_chunk: invariant violated: %s", #COND); return ORBX_ERR_UNSUPPORTED; } \
    } while (0)

static inline int plan_chunk(const PlanInput &in, ChunkPlan *out) {
    const int32_t *opt = in.opt;
    const int B = in.B, nl = in.nl;
    const unsigned allLevels = (1u << nl) - 1u;
    ChunkPlan p = {};
    p.fastPhase = opt[0]; p.octPhase = opt[1]; p.octStop = opt[7]; p.descLdsPad = opt[21] * 1024;
    // With the pyramid built ahead nothing but a stream wait (for that pyramid) sits in front of the FAST launch, and a timing
    // event recorded right behind a pending wait can be stamped before the wait is over: the bracket then reads wait + FAST
    // (seen as 0.30 instead of 0.27 ms in one run out of four).  An empty kernel orders the stamp behind the wait.
    p.orderKernel = in.profFast && in.skipPyr && opt[12] == 0;
    // a pyramid built ahead starts behind this call's FAST stage (ORBX_OPT_PREFETCH_GATE: 1 behind the quad-tree, 2 behind the
    // descriptors, 3 as soon as this FAST stage may start - it then runs beside it)
    p.fastDoneAt = in.pfUsed && !in.evPyrDone ? opt[10] : ORBX_FASTDONE_NEVER;

    // ---- FAST.  ORBX_OPT_FAST_FORM: 1 = every level by k_fast_cells (compile-time tile strides), 2 = ... with run-time strides, 3 = strips.
    // A strip is a longer job than a cell (a wave walks ~33 rows): with few images the one-wave-per-cell kernel finishes
    // sooner (13 vs 29 us for one 1241x376 image); once the strips fill the GPU they win (2.5 vs 3.1 us per image).  Same results.
    p.strips = in.totalStrips > 0 && (opt[6] == 0 ? (long long)in.totalStrips * B >= 4096 : opt[6] == 3);
    p.stripLevels = p.strips ? in.stripLevels : 0;
    p.fastCells = (unsigned)p.stripLevels != allLevels;   // levels with wider cells (the coarsest ones of small images)
    // the strides of the usual 30-px cell grids; anything else takes the run-time-stride instance
    const int es = in.fastScoreStride == in.fastTileStride - 8 && opt[6] != 2 ? in.fastTileStride : 0;
    p.es = es == 44 || es == 48 || es == 52 ? es : 0;

    // ---- quad-tree input.  ORBX_OPT_OCTREE_FORM: 0 default, 1 = the exact form alone, 2 = EVERY level by the multi-workgroup form, 3 = none.
    p.usePyr = opt[4] != 1;
    // ORBX_OPT_OCT_HIST (0 = by batch size, 1 = never): with at most ORBX_HIST_IMAGES images and every level done by k_fast_cells, the FAST
    // stage histograms its emissions for the quad-tree (FastHist) and k_octree_pyr loads the histogram instead of sweeping the keys: no
    // shared sweep is needed at all (one 1920x1080 image went through gather 6 + k_octree_big 53 + 15 us)
    const bool histWanted = opt[23] == 0 && B <= ORBX_HIST_IMAGES && in.lastChunks == 1 && !p.strips && opt[0] == 0 && opt[18] != 1 &&
                            opt[7] == 0 && opt[1] == 0;
    // The multi-workgroup form shortens ONE image's critical path (a 1920x1080 level 0: 195 us alone in its workgroup); a
    // batch already fills the GPU with one workgroup per (image, level), and the extra hand-offs then cost more than they save
    // (batch 32 of 1920x1080: 274 us against 215), so it is taken for small batches only.  Same results either way.
    p.multiWg = opt[4] == 2 || (opt[4] != 3 && B <= 4 && in.octBigMask != 0 && !histWanted);
    // Fused: k_octree_pyr reads the FAST stage's cell lists in place (no k_gather launch, no compacted key array: -35 us per
    // 128 images 1241x376, -200 us per 64 images 1920x1080 in the pipelined step).  Not for the multi-workgroup form, the exact
    // form alone and the phase-stop knobs, which sweep the compacted array (ORBX_OPT_GATHER = 1: never fused).
    p.fused = p.usePyr && !p.multiWg && (opt[7] == 0 || opt[7] == 8 || opt[7] == 9) && opt[1] == 0 && opt[18] != 1;   // (7 = 8 / 9, developer build: time stamps, no stop)
    p.gather = !p.fused;
    p.histOct = p.fused && histWanted;
    // (only the multi-workgroup form shares levels: it sweeps the COMPACTED keys, which exist only when k_gather ran)
    p.bigMask = !(p.usePyr && p.multiWg) ? 0 : opt[4] == 2 ? (int32_t)allLevels : in.octBigMask;
    // 1024-thread instances for images with a large level (>= 600 FAST cells; ORBX_OPT_OCTREE_WIDTH: 1 = never, 2 = always)
    p.wideOct = opt[11] == 0 ? in.octBigMask != 0 : opt[11] == 2;

    // ---- corner-sparse levels.  ORBX_OPT_ROW_PRETEST: 1 = never the sparse path, 2 = always.
    p.sparsePerCell = opt[16] == 2 ? 1 << 20 : ORBX_SPARSE_PER_CELL;
    p.rowFlags = p.strips && opt[16] != 1;
    // ORBX_OPT_SPARSE_FORM 1 / 2 (alternatives, measured no faster than the default row skip inside the strip kernel - DESIGN.md
    // section 5): the corner-sparse (image, level)s - flagged by the previous call's quad-tree - leave the strip kernel and are done
    // by a compaction kernel.  That costs a launch whose waves all return at once when nothing is flagged, so it is added
    // only while the handle has recently met a sparse level: the quad-tree of image slot 0 stores the call's sequence number
    // into a host-mapped word when it flags one (a hint that lags by the calls in flight; a wrong hint costs speed only,
    // because both kernels take the SAME device flags).
    p.sparseForm = opt[20];
    p.compact = p.rowFlags && opt[20] != 0 && (opt[16] == 2 || in.sparseRecent);
    p.sparseHint = opt[20] == 0 ? ORBX_HINT_NONE : p.fused ? ORBX_HINT_OCT_SRC : ORBX_HINT_GATHER;   // (the hint only serves the compaction forms)

    // ---- arrangements of a batch that fills the GPU (both off by default: measured slower)
    // Early quad-tree (ORBX_OPT_EARLY_OCTREE: a >= 2 = levels [0, a)): the quad-tree of the large levels is ONE workgroup per level walking a
    // serial chain - the critical path behind FAST.  Their strips go first, in a launch of their own, and their quad-tree starts on a
    // second stream as soon as that launch is done, beside the FAST of the remaining levels.  (64 stereo frames 1241x376: 0.635 -> 0.649 ms
    // per step with a = 2, 0.657 with a = 3; 2000 features 0.838 -> 0.874; 1920x1080 x 64 1.254 -> 1.274; 752x480 0.599 -> 0.607: FAST
    // loses to the quad-tree workgroups what the shorter chain behind it gains, plus two cross-stream events.)
    const int ea = opt[19];
    const unsigned eaMask = ea >= 2 && ea < 32 ? (1u << ea) - 1u : 0u;
    if (p.strips && p.fused && !in.prof && !p.compact && ea >= 2 && opt[15] < 2 && in.lastChunks == 1 && B >= 8 && nl > ea &&
        ((unsigned)in.stripLevels & eaMask) == eaMask && !in.dbgBlur)
        p.earlyLv = ea;
    // Split call (ORBX_OPT_SPLIT_CALL: a >= 2 = at level a): the quad-tree of the levels [0, a) on a second stream beside the quad-tree and
    // the descriptors of the levels [a, nl)
    if (p.usePyr && !in.prof && in.lastChunks == 1 && B >= 8 && opt[7] == 0 && opt[1] == 0 && opt[15] >= 2 && !p.multiWg && !in.dbgBlur && nl >= 3)
        p.aSplit = std::min(opt[15], nl - 1);

    // ---- the quad-tree form
    int nBig = 0;
    for (int l = 0; l < nl; l++) nBig += ((unsigned)p.bigMask >> l) & 1u;
    p.octForm = !p.usePyr ? ORBX_OCT_EXACT
              : nBig > 0 && opt[7] == 0 && opt[1] == 0 ? ORBX_OCT_BIG
              : p.earlyLv > 0 ? ORBX_OCT_EARLY
              : p.aSplit > 0 ? ORBX_OCT_SPLIT : ORBX_OCT_SINGLE;   // (single: no large level, or a phase-stop knob is set)
    // ... except that in a BATCH the sweep of a large level (>= 600 FAST cells) MAY be shared by two or four workgroups
    // (ORBX_OPT_OCT_SLICES = 1; off by default): the level-0 workgroup of a 1920x1080 image is the critical path of the stage
    // (113 us, 64 of them its sweep), and sharing the sweeps takes the stage ALONE from 120 to 90 us at batch 32 - but the pipelined
    // step gets slower (0.6105 -> 0.6277 ms at batch 32, 1.186 -> 1.256 ms at batch 64): beside the next pyramid and the previous
    // matcher the extra 1024-thread workgroups cost more than the shorter critical path gives back
    if (p.octForm == ORBX_OCT_SINGLE && p.fused && !p.histOct && opt[26] == 1 && in.sliceScratch && opt[7] == 0 && opt[1] == 0) {
        p.sweepSlices = 1;
        for (int l = 0; l < nl; l++) {
            p.nslice[l] = in.ncells[l] >= 1600 ? 4 : in.ncells[l] >= 600 ? 2 : 1;
            p.sweepShared |= p.nslice[l] > 1;
        }
    }

    // ---- what the kernels rely on
    ORBX_PLAN_NEEDS(p.gather == !p.fused);
    ORBX_PLAN_NEEDS(plan_implies(p.multiWg, !p.fused));   // the multi-workgroup form sweeps the compacted keys: k_gather must have run
    ORBX_PLAN_NEEDS(plan_implies(p.bigMask != 0, p.multiWg));
    ORBX_PLAN_NEEDS(plan_implies(p.histOct, p.fused && !p.strips && B <= ORBX_HIST_IMAGES && in.lastChunks == 1 && !p.multiWg));
    ORBX_PLAN_NEEDS(plan_implies(p.earlyLv > 0, p.fused && p.strips && !p.compact && p.aSplit == 0 && !in.prof &&
                                                    ((unsigned)p.stripLevels & eaMask) == eaMask));
    ORBX_PLAN_NEEDS(plan_implies(p.aSplit > 0, p.usePyr && !p.multiWg && nl >= 3 && p.aSplit < nl));
    ORBX_PLAN_NEEDS(plan_implies(p.sweepSlices || p.sweepShared, p.fused && !p.histOct && in.sliceScratch && p.octForm == ORBX_OCT_SINGLE));
    ORBX_PLAN_NEEDS((p.octForm == ORBX_OCT_EXACT) == !p.usePyr);
    ORBX_PLAN_NEEDS(plan_implies(p.octForm == ORBX_OCT_BIG, p.multiWg && p.bigMask != 0 && opt[1] == 0 && opt[7] == 0));
    ORBX_PLAN_NEEDS(plan_implies(p.octForm == ORBX_OCT_EARLY, p.earlyLv > 0) && plan_implies(p.octForm == ORBX_OCT_SPLIT, p.aSplit > 0));
    ORBX_PLAN_NEEDS(plan_implies(p.earlyLv > 0, p.octForm == ORBX_OCT_EARLY) && plan_implies(p.aSplit > 0, p.octForm == ORBX_OCT_SPLIT));
    ORBX_PLAN_NEEDS(plan_implies(!p.fused, p.sparseHint != ORBX_HINT_OCT_SRC) && plan_implies(p.fused, p.sparseHint != ORBX_HINT_GATHER));
    *out = p;
    return ORBX_OK;
}
