// orbx_size_plan.h — everything an extractor derives from an image size: level geometry, cv::resize coefficient tables, quad-tree
// root and path tables, pyramid tile spans, strip numbering, LDS sizes.  plan_size is plain C++ (no HIP call, no handle): ensure_plan
// (orbx_extract.hip) builds a SizeInput, gets a SizePlan and only allocates and uploads; a size the kernels cannot take is refused
// here, before anything of the handle is touched.  Every rule is stated ONCE.  Included by orbx_internal.h (the handle keeps its
// SizePlan); the developer build's orbx_debug_size_plan (include/orbx_dev.h) hands the plan out without a GPU.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "orbx.h"

#define ORBX_MAX_LEVELS 16
#define ORBX_EDGE 19        // EDGE_THRESHOLD            (reference: src/ORBextractor.cc:74)
#define ORBX_MINB 16        // minBorderX = EDGE-3       (reference: src/ORBextractor.cc:773)
#define ORBX_HALF_PATCH 15  // HALF_PATCH_SIZE           (reference: src/ORBextractor.cc:73)
#define ORBX_MAX_ROOTS 64

void orbx_set_error(const char *fmt, ...);
// what the kernels can take
#define ORBX_LDS_LIMIT (150 * 1024)       // dynamic LDS of one workgroup (of the 160 KiB of a CU)
#define ORBX_CHAIN_LDS_LIMIT (60 * 1024)  // k_pyr_chain: two workgroups per CU
#define ORBX_CHAIN_MAX_COLS 128           // k_pyr_chain: widest level tile (two columns per lane)
#define ORBX_MAX_CELL_WINDOW 65           // k_fast_cells: a FAST cell with its 3-px halo, per axis
#define ORBX_MAX_COORD 4095               // candidate coordinates are packed in 12 bits
#define ORBX_MAX_KEYS 0xFFFFFF            // best-key election packs (response << 24 | ~index) in one LDS word
#define ORBX_PYR_MAX_CELLS 16384          // cell codes of the quad-tree count pyramid are 16-bit path-table entries

// Per-level geometry, built on the host (exactly the reference's arithmetic) and read by
// every kernel from device memory.
struct LevelGeom {
    int w, h;            // inner level size: cvRound(cols*inv), cvRound(rows*inv)   (:1111-1112)
    int pstride, prows;  // padded buffer: row stride in bytes (multiple of 64), rows = h+38
    unsigned long long poff;  // byte offset of the padded level inside one image's pyramid block
    int regW, regH;      // maxBorderX-minBorderX, maxBorderY-minBorderY                 (:773-781)
    int nCols, nRows, wCell, hCell;  //                                                  (:784-787)
    int cellBase, ncells;            // global cell numbering across levels
    int capc;                        // candidate slots per cell = ceil(wCell/2)*ceil(hCell/2)
    unsigned long long slotOff;      // uint32 offset of this level's slots inside one image's slot block
    int N;                           // mnFeaturesPerLevel[level]
    int nIni;                        // round(regW/regH)                                  (:543)
    int nodeCap;                     // quad-tree list capacity N + 3 + 4*nIni
    int pyrDepth;                    // depth Dm of the quad-tree count pyramid (k_octree_pyr)
    unsigned long long keyOff;       // element offset of this level's keys inside one image's key block
    int keyCap;                      // ncells*capc
    int lvlKpOff;                    // offset of this level's kept keypoints in the per-image list
    int xofsOff, xalphaOff, yofsOff, ybetaOff;  // resize tables (int32 units into d_tab), levels >= 1
    int rootTabOff, rootBoxOff;      // byte offset (uint8 rootOf[x]) / int32 offset (root x bounds)
    int xPathOff, yPathOff;          // int32 offsets: quad-tree path of a key at depth pyrDepth, per x (root<<2D | even bits) / per y (odd bits)
    float scale;                     // mvScaleFactor[level]
    float size;                      // (float)(int)(31*scale)                            (:837,846)
};

// One launch of k_pyr_chain (orbx_extract_dev.h): up to PC_MAXL consecutive pyramid levels built from the level in front of them
#define PC_MAXL 7
struct ChainPlan {
    int la, lb;                  // source level, last level built (lb - la <= PC_MAXL)
    int tilesX, tilesY;
    int xSpanOff, ySpanOff;      // int32 offsets into tab: PyrSpan [lb - la + 1][tiles] per axis (level la first)
    int bufBytes, maxRows;       // one LDS level buffer, rows of the ypar table per level
};

static inline int cv_round(double v) { return (int)lrint(v); }
static inline int cv_floor(double v) { int i = (int)v; return i - (v < i); }
static inline int cv_ceil(double v) { int i = (int)v; return i + (v > i); }
static inline short sat_short_round(float v) {
    int i = cv_round(v);
    return (short)(i < -32768 ? -32768 : i > 32767 ? 32767 : i);
}

// The tables of ORBextractor's constructor: they depend on (nfeatures, scale_factor, nlevels) alone.
struct ExtractorTables {
    float sf[ORBX_MAX_LEVELS], isf[ORBX_MAX_LEVELS], sig2[ORBX_MAX_LEVELS], isig2[ORBX_MAX_LEVELS];
    int32_t nfeat[ORBX_MAX_LEVELS], umax[16];
};
static inline void extractor_tables(int nfeatures, double scale_factor, int nlevels, ExtractorTables *t) {
    // scale tables (:415-431)
    t->sf[0] = 1.0f; t->sig2[0] = 1.0f;
    for (int i = 1; i < nlevels; i++) {
        t->sf[i] = (float)(t->sf[i - 1] * scale_factor);
        t->sig2[i] = t->sf[i] * t->sf[i];
    }
    for (int i = 0; i < nlevels; i++) { t->isf[i] = 1.0f / t->sf[i]; t->isig2[i] = 1.0f / t->sig2[i]; }
    // features per level (:435-446)
    float factor = (float)(1.0f / scale_factor);
    float nDesired = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels));
    int sum = 0;
    for (int level = 0; level < nlevels - 1; level++) {
        t->nfeat[level] = cv_round(nDesired);
        sum += t->nfeat[level];
        nDesired *= factor;
    }
    t->nfeat[nlevels - 1] = std::max(nfeatures - sum, 0);
    // umax (:454-469)
    int v, v0, vmax = cv_floor(ORBX_HALF_PATCH * sqrtf(2.f) / 2 + 1);
    int vmin = cv_ceil(ORBX_HALF_PATCH * sqrtf(2.f) / 2);
    const double hp2 = ORBX_HALF_PATCH * ORBX_HALF_PATCH;
    for (v = 0; v <= vmax; ++v) t->umax[v] = cv_round(sqrt(hp2 - v * v));
    for (v = ORBX_HALF_PATCH, v0 = 0; v >= vmin; --v) {
        while (t->umax[v0] == t->umax[v0 + 1]) ++v0;
        t->umax[v] = v0;
        ++v0;
    }
}

struct SizeInput {   // everything plan_size reads
    int w, h, nlevels;
    double scale_factor;
    ExtractorTables tb;
    int pyrTile;     // ORBX_OPT_PYRAMID_TILE (option 3): level-0 pixels per fused-pyramid tile, 0 = 64
};
struct SizePlan {    // everything that depends on the image size
    LevelGeom geom[ORBX_MAX_LEVELS];
    std::vector<int32_t> tab;   // resize, root, path and span tables (LevelGeom::*Off, pyr*SpanOff, ChainPlan::*SpanOff index it)
    int max_kp;                 // keypoints one image can return
    int totalCells, maxNodeCap, lvlKpCap;
    size_t pyrImgBytes, slotsPerImg, keysPerImg;
    int fastTileStride, fastScoreStride, fastTileRows, fastLdsPerWave;
    int stripBase[ORBX_MAX_LEVELS + 1], totalStrips;   // k_fast_strips: first strip of every level, strips per image
    unsigned stripLevels;                              // bit l: level l is k_fast_strips' (cells <= 32 px wide), else k_fast_cells'
    size_t octLdsBytes, octPyrLdsBytes; int octPyrWords;
    unsigned octBigMask; int octDeepMax;               // levels with >= 600 FAST cells (multi-workgroup quad-tree), its count partials
    int octSliceStride;                                // shared sweeps of large levels in a batch (OctSrc::nslice); 0: no such level
    int histStride;                                    // deepest-depth histogram of small batches (FastHist)
    int pyrTilesX, pyrTilesY, pyrXSpanOff, pyrYSpanOff, pyrBufBytes, pyrMaxDim, pyrMaxPar;
    size_t pyrLdsBytes;
    ChainPlan chains[2][8]; int nChains[2];   // level chains of small batches (k_pyr_chain): [0] up to 4 levels per chain, [1] up to PC_MAXL
};

// Depth of a level's quad-tree count pyramid: enough cells for the passes of a dense level (4 N, at most depth 7), bounded by the
// cell cap (a level that needs more depth than its pyramid has is redone by the exact form inside the same workgroup, so the cap
// costs speed only)
static inline int pyr_depth(int nIni, int N, int cellCap) {
    int d = 1;
    while ((nIni << (2 * d)) < 4 * std::max(N, 1) && d < 7) d++;
    while ((nIni << (2 * d)) > cellCap && d > 1) d--;
    return d;
}
static inline int pyr_deep_cells(const LevelGeom &g) { return g.nIni << (2 * g.pyrDepth); }
// Bytes of one image a caller hands over in level 0's own layout (orbx_level0_layout): the padded level, plus 64 bytes so that a
// load that starts on the level's last dword may be up to 16 bytes wide wherever the image sits in the caller's allocation (inside the
// pyramid block the next level follows), rounded up to the 256 bytes the pyramid block's images are apart by
static inline size_t level0_image_bytes(const LevelGeom &g0) { return ((size_t)g0.pstride * g0.prows + 64 + 255) & ~(size_t)255; }
static inline size_t pow2_at_least(int n) { size_t p = 1; while (p < (size_t)n) p <<= 1; return p; }
// Dynamic LDS of k_octree_pyr, term by term as octree_pyr_body carves it (orbx_octree.hip:233-241, :252, :264-265): the sort keys;
// per list node cntA 8 + nidA 8 + hist 16 + pn 4 + xlist 2 + split 1; the count pyramid; the 16-bit path tables (regW + regH); the
// best-key pyramid; cellOff[ncells + 1]; alignment slack
static inline size_t oct_pyr_lds_bytes(int nodeCap, int pyrWords, int pathLen, int bestWords, int cells) {
    return sizeof(unsigned long long) * pow2_at_least(nodeCap) + (size_t)nodeCap * (8 + 8 + 16 + 4 + 2 + 1) + 4 * (size_t)pyrWords +
           2 * (size_t)pathLen + 4 * (size_t)bestWords + 4 * (size_t)(cells + 1) + 64 + 8;
}
// Dynamic LDS of the exact form, as octree_exact_level carves it (orbx_octree.hip:886-899): the sort keys; per list node box 2 x 8 +
// cnt 2 x 4 + pn 4 + pg 4 + childIdx 4 x 2 + survIdx 2 + xlist 2 + split 1; hist[max(4 cap, ncells + 1)]; alignment slack
static inline size_t oct_exact_lds_bytes(int nodeCap, int cells) {
    return sizeof(unsigned long long) * pow2_at_least(nodeCap) + (size_t)nodeCap * (8 * 2 + 4 * 2 + 4 * 2 + 2 * 4 + 2 + 2 + 1) +
           4 * (size_t)std::max(4 * nodeCap, cells + 1) + 64;
}

// Tile spans of one axis (0 = x, 1 = y) of a pyramid kernel that builds the levels la+1 .. lb from level la in tiles of T pixels of
// level lb: own_l partitions level l, comp_l = own_l + the rows / columns of level l that comp_{l+1} reads through xofs / yofs.
// Appends PyrSpan (4 shorts = 2 int32: own0, own1, comp0, comp1) [lb - la + 1][tiles] to tab, level la first; returns the tile count.
// widest[l - la] takes the widest compute span of level l, *maxPar the largest sum of a tile's compute spans (both are maxima:
// they keep what they hold).
static inline int plan_spans(const LevelGeom *geom, std::vector<int32_t> &tab, int la, int lb, int T, int axis, int *spanOff, int *widest,
                             int *maxPar) {
    auto dim = [&](int l) { return axis == 0 ? geom[l].w : geom[l].h; };
    const int dc = dim(lb), nt = (dc + T - 1) / T;
    const size_t off = tab.size();
    tab.resize(off + (size_t)2 * (lb - la + 1) * nt);
    *spanOff = (int)off;
    for (int t = 0; t < nt; t++) {
        int c0 = 0, c1 = 0, parSum = 0;
        for (int l = lb; l >= la; l--) {
            const int d = dim(l);
            const int b0 = std::min(t * T, dc), b1 = std::min((t + 1) * T, dc);
            const int o0 = (int)((long long)b0 * d / dc), o1 = (t == nt - 1) ? d : (int)((long long)b1 * d / dc);
            if (l == lb) { c0 = o0; c1 = o1; }
            else {   // rows / cols of level l read by comp_{l+1} = [c0, c1)
                const LevelGeom &gn = geom[l + 1];
                const int ofsOff = axis == 0 ? gn.xofsOff : gn.yofsOff;
                int n0 = tab[ofsOff + c0], n1 = tab[ofsOff + c1 - 1] + 1;
                n0 = std::min(std::max(n0, 0), d - 1);
                n1 = std::min(std::max(n1, 0), d - 1);
                c0 = std::min(n0, o0);
                c1 = std::max(n1 + 1, o1);
            }
            short *e = (short *)&tab[off] + 4 * ((size_t)(l - la) * nt + t);
            e[0] = (short)o0; e[1] = (short)o1; e[2] = (short)c0; e[3] = (short)c1;
            widest[l - la] = std::max(widest[l - la], c1 - c0);
            parSum += c1 - c0;
        }
        *maxPar = std::max(*maxPar, parSum);
    }
    return nt;
}

// (w, h) -> SizePlan.  ORBX_ERR_ARG: a level is smaller than a FAST cell or has no quad-tree root; ORBX_ERR_UNSUPPORTED: a limit of the
// kernels (above).  *out is written only on ORBX_OK.
static inline int plan_size(const SizeInput &in, SizePlan *out) {
    const int nl = in.nlevels;
    const ExtractorTables &tb = in.tb;
    SizePlan p = {};
    std::vector<int32_t> &tab = p.tab;
    size_t poff = 0, slotOff = 0, keyOff = 0;
    int cellBase = 0, lvlKpOff = 0, maxCells = 0, maxPath = 0, maxTw = 0, maxTh = 0;
    // ---- level geometry (:773-787, :1111-1112) and what it can be refused for
    for (int l = 0; l < nl; l++) {
        LevelGeom &g = p.geom[l];
        const float scale = tb.isf[l];
        g.w = cv_round((float)in.w * scale);
        g.h = cv_round((float)in.h * scale);
        g.regW = g.w - 2 * ORBX_MINB;
        g.regH = g.h - 2 * ORBX_MINB;
        if (g.regW < 30 || g.regH < 30) {
            orbx_set_error("level %d is %dx%d: the reference needs (w-32)>=30 and (h-32)>=30 at every level "
                           "(nCols/nRows would be 0, src/ORBextractor.cc:784-787)", l, g.w, g.h);
            return ORBX_ERR_ARG;
        }
        if (g.w > ORBX_MAX_COORD || g.h > ORBX_MAX_COORD) {
            orbx_set_error("image %dx%d too large: candidate coordinates are packed in 12 bits", in.w, in.h);
            return ORBX_ERR_UNSUPPORTED;
        }
        g.pstride = (g.w + 2 * ORBX_EDGE + 63) & ~63;
        g.prows = g.h + 2 * ORBX_EDGE;
        g.poff = poff;
        poff += (size_t)g.pstride * g.prows;
        const float W = 30;
        const float width = (float)g.regW, height = (float)g.regH;
        g.nCols = (int)(width / W);
        g.nRows = (int)(height / W);
        g.wCell = (int)ceilf(width / g.nCols);
        g.hCell = (int)ceilf(height / g.nRows);
        g.ncells = g.nCols * g.nRows;
        g.cellBase = cellBase;
        cellBase += g.ncells;
        g.capc = ((g.wCell + 1) / 2) * ((g.hCell + 1) / 2);
        g.slotOff = slotOff;
        slotOff += (size_t)g.ncells * g.capc;
        g.keyOff = keyOff;
        g.keyCap = g.ncells * g.capc;
        if (g.keyCap > ORBX_MAX_KEYS) {
            orbx_set_error("level %d can hold %d FAST candidates (> 2^24): unsupported", l, g.keyCap);
            return ORBX_ERR_UNSUPPORTED;
        }
        keyOff += ((size_t)g.keyCap + 7) & ~(size_t)7;  // 16-B aligned key blocks (uint4 / ushort4 sweeps)
        g.N = tb.nfeat[l];
        g.nIni = (int)roundf((float)g.regW / g.regH);
        if (g.nIni < 1 || g.nIni > ORBX_MAX_ROOTS) {
            orbx_set_error("aspect ratio gives %d quad-tree roots at level %d (reference divides by zero "
                           "below 1; supported up to %d)", g.nIni, l, ORBX_MAX_ROOTS);
            return g.nIni < 1 ? ORBX_ERR_ARG : ORBX_ERR_UNSUPPORTED;
        }
        g.nodeCap = std::max(g.N + 3, 4 * g.nIni) + 4 * g.nIni + 1;
        // a level with this many FAST cells carries tens of thousands of keys: in a small batch its quad-tree is shared by several
        // workgroups (single image, orbx_extract host to host: 1920x1080 / 4000 features 418 -> 348 us).  Smaller levels gain
        // nothing reliable: with every level >= 100 cells shared, 1241x376 / 1000 features went 184 -> 176 us, / 2000 features 225 -> 233 us
        if (g.ncells >= 600) p.octBigMask |= 1u << l;
        p.max_kp += std::max(g.N + 2, 4 * g.nIni);   // every level returns at most max(N+2, 4*nIni) nodes
        p.maxNodeCap = std::max(p.maxNodeCap, g.nodeCap);
        maxCells = std::max(maxCells, g.ncells);
        maxPath = std::max(maxPath, g.regW + g.regH);   // the level's path tables ride in LDS (k_octree_pyr / k_octree_big)
        g.lvlKpOff = lvlKpOff;
        lvlKpOff += g.nodeCap;
        g.scale = tb.sf[l];
        g.size = (float)(int)(31 * tb.sf[l]);
        maxTw = std::max(maxTw, g.wCell + 6);
        maxTh = std::max(maxTh, g.hCell + 6);
    }
    // ---- depth of the quad-tree count / best-key pyramids: under the largest cell cap with which k_octree_pyr fits its LDS budget
    for (int cellCap = ORBX_PYR_MAX_CELLS;; cellCap >>= 2) {
        int maxBestWords = 0;
        p.octPyrWords = 0;
        for (int l = 0; l < nl; l++) {
            LevelGeom &g = p.geom[l];
            const int d = g.pyrDepth = pyr_depth(g.nIni, g.N, cellCap);
            p.octPyrWords = std::max(p.octPyrWords, g.nIni * (((1 << (2 * d)) - 1) / 3) + (pyr_deep_cells(g) + 1) / 2 + 1);
            maxBestWords = std::max(maxBestWords, g.nIni * (((1 << (2 * (d + 1))) - 1) / 3));
        }
        p.octPyrLdsBytes = oct_pyr_lds_bytes(p.maxNodeCap, p.octPyrWords, maxPath, maxBestWords, maxCells);
        if (p.octPyrLdsBytes <= ORBX_LDS_LIMIT || cellCap <= 64) break;
    }
    for (int l = 0; l < nl; l++) {
        const int deep = pyr_deep_cells(p.geom[l]);
        p.octDeepMax = std::max(p.octDeepMax, (deep + 1) / 2 + 1);
        p.histStride = std::max(p.histStride, (deep + 3) & ~3);
        if (p.geom[l].ncells >= 600) p.octSliceStride = std::max(p.octSliceStride, deep);
    }
    // ---- the tables of every level
    for (int l = 0; l < nl; l++) {
        LevelGeom &g = p.geom[l];
        // resize tables of cv::resize(INTER_LINEAR, 8UC1) from level l-1
        if (l > 0) {
            const int sw = p.geom[l - 1].w, shh = p.geom[l - 1].h;
            const double inv_scale_x = (double)g.w / sw, inv_scale_y = (double)g.h / shh;
            const double scale_x = 1. / inv_scale_x, scale_y = 1. / inv_scale_y;
            g.xofsOff = (int)tab.size();
            tab.resize(tab.size() + g.w);
            g.xalphaOff = (int)tab.size();
            tab.resize(tab.size() + g.w);
            for (int dx = 0; dx < g.w; dx++) {
                float fx = (float)((dx + 0.5) * scale_x - 0.5);
                int sx = cv_floor(fx);
                fx -= sx;
                if (sx < 0) { fx = 0; sx = 0; }
                if (sx >= sw - 1) { fx = 0; sx = sw - 1; }
                const short a0 = sat_short_round((1.f - fx) * 2048), a1 = sat_short_round(fx * 2048);
                tab[g.xofsOff + dx] = sx;
                tab[g.xalphaOff + dx] = (int32_t)((uint32_t)(uint16_t)a0 | ((uint32_t)(uint16_t)a1 << 16));
            }
            g.yofsOff = (int)tab.size();
            tab.resize(tab.size() + g.h);
            g.ybetaOff = (int)tab.size();
            tab.resize(tab.size() + g.h);
            for (int dy = 0; dy < g.h; dy++) {
                float fy = (float)((dy + 0.5) * scale_y - 0.5);
                int sy = cv_floor(fy);
                fy -= sy;
                const short b0 = sat_short_round((1.f - fy) * 2048), b1 = sat_short_round(fy * 2048);
                tab[g.yofsOff + dy] = sy;
                tab[g.ybetaOff + dy] = (int32_t)((uint32_t)(uint16_t)b0 | ((uint32_t)(uint16_t)b1 << 16));
            }
        }
        // quad-tree roots (:543-569): boxes and the key -> root map, tabulated in host float
        const float hX = (float)g.regW / g.nIni;
        g.rootBoxOff = (int)tab.size();
        for (int i = 0; i <= g.nIni; i++) tab.push_back((int)(hX * (float)i));
        const int words = (g.regW + 3) / 4;
        g.rootTabOff = (int)(tab.size() * 4);
        const size_t base = tab.size();
        tab.resize(tab.size() + words, 0);
        uint8_t *rt = (uint8_t *)&tab[base];
        for (int x = 0; x < g.regW; x++) {
            size_t r = (size_t)((float)x / hX);
            if (r >= (size_t)g.nIni) r = g.nIni - 1;
            rt[x] = (uint8_t)r;
        }
        // DivideNode splits x and y independently (:483-484, :513-525), so the path of a key down to depth
        // pyrDepth is (bits decided by x alone) interleaved with (bits decided by y alone): two lookups
        // replace pyrDepth rounds of box arithmetic per key in k_octree_pyr.  Cell code at depth d =
        // (xPath[x] | yPath[y]) >> 2*(pyrDepth - d), child index = xbit | ybit << 1 like child_of().
        const int D = g.pyrDepth;
        g.xPathOff = (int)tab.size();
        for (int x = 0; x < g.regW; x++) {
            const int r = ((const uint8_t *)&tab[base])[x];
            int lo = tab[g.rootBoxOff + r], hi = tab[g.rootBoxOff + r + 1];
            uint32_t path = 0;
            for (int d = 0; d < D; d++) {
                const int mx = lo + ((hi - lo + 1) >> 1);
                const uint32_t bit = x < mx ? 0u : 1u;
                if (bit) lo = mx; else hi = mx;
                path = (path << 2) | bit;
            }
            tab.push_back((int32_t)(((uint32_t)r << (2 * D)) | path));
        }
        g.yPathOff = (int)tab.size();
        for (int y = 0; y < g.regH; y++) {
            int lo = 0, hi = g.regH;
            uint32_t path = 0;
            for (int d = 0; d < D; d++) {
                const int my = lo + ((hi - lo + 1) >> 1);
                const uint32_t bit = y < my ? 0u : 1u;
                if (bit) lo = my; else hi = my;
                path = (path << 2) | (bit << 1);
            }
            tab.push_back((int32_t)path);
        }
    }
    {   // ---- fused pyramid (k_pyramid_fused): every level from level 0, in tiles of the coarsest level
        const int Lc = nl - 1;
        int T = (int)lrintf((in.pyrTile > 0 ? (float)in.pyrTile : 64.0f) / tb.sf[Lc]);
        T = std::max(4, std::min(64, (T + 2) & ~3));
        int widest[ORBX_MAX_LEVELS] = {}, maxPar = 0;
        p.pyrTilesX = plan_spans(p.geom, tab, 0, Lc, T, 0, &p.pyrXSpanOff, widest, &maxPar);
        p.pyrTilesY = plan_spans(p.geom, tab, 0, Lc, T, 1, &p.pyrYSpanOff, widest, &maxPar);
        p.pyrMaxDim = (*std::max_element(widest, widest + nl) + 3) & ~3;
        p.pyrBufBytes = (p.pyrMaxDim * p.pyrMaxDim + 15) & ~15;
        p.pyrMaxPar = (maxPar + 3) & ~3;
        p.pyrLdsBytes = 2 * (size_t)p.pyrBufBytes + (size_t)p.pyrMaxPar * 16 + 16;
        if (p.pyrLdsBytes > ORBX_LDS_LIMIT) { orbx_set_error("pyramid tile needs %zu B of LDS", p.pyrLdsBytes); return ORBX_ERR_UNSUPPORTED; }
    }
    for (int variant = 0; variant < 2; variant++) {   // ---- level chains of small batches (ChainPlan): levels 1 .. nlevels-1 in groups of up to
        // CL levels, the first group the short one - planned twice: chains of up to 4 levels (variant 0) and of up to PC_MAXL = 7 (variant 1)
        const int CL = variant == 0 ? 4 : PC_MAXL;
        const int nbTotal = nl - 1;
        if (nbTotal < 1 || !(in.scale_factor <= 2.0)) continue;
        const int nch = (nbTotal + CL - 1) / CL;
        bool ok = true;
        for (int c = 0, la = 0; c < nch && ok; c++) {
            const int nb = c == 0 ? nbTotal - CL * (nch - 1) : CL, lb = la + nb;
            ChainPlan cp = {};
            cp.la = la; cp.lb = lb;
            const int TY = nb <= 4 ? 8 : 16;   // (long chains: taller tiles, less of the accumulated row halo per owned row)
            bool fits = false;
            for (int TX = 96; TX >= 16 && !fits; TX -= 4) {
                const size_t mark = tab.size();
                int cw[PC_MAXL + 1] = {}, chh[PC_MAXL + 1] = {}, par = 0;
                cp.tilesX = plan_spans(p.geom, tab, la, lb, TX, 0, &cp.xSpanOff, cw, &par);
                cp.tilesY = plan_spans(p.geom, tab, la, lb, TY, 1, &cp.ySpanOff, chh, &par);
                int buf = 0, maxW = 0, maxRows = 0;
                for (int k = 0; k <= nb; k++) {
                    if (k > 0) { maxW = std::max(maxW, cw[k]); maxRows = std::max(maxRows, chh[k]); }
                    buf = std::max(buf, ((cw[k] + 8 + 3) & ~3) * chh[k]);
                }
                cp.bufBytes = (buf + 15) & ~15;
                cp.maxRows = maxRows;
                fits = maxW <= ORBX_CHAIN_MAX_COLS && 2 * (size_t)cp.bufBytes + (size_t)nb * maxRows * 8 <= ORBX_CHAIN_LDS_LIMIT;
                if (!fits) tab.resize(mark);
            }
            ok = fits;
            if (ok) p.chains[variant][p.nChains[variant]++] = cp;
            la = lb;
        }
        if (!ok) p.nChains[variant] = 0;
    }
    if (maxTw > ORBX_MAX_CELL_WINDOW || maxTh > ORBX_MAX_CELL_WINDOW) { orbx_set_error("cell window %dx%d exceeds 65", maxTw, maxTh); return ORBX_ERR_UNSUPPORTED; }
    // ---- k_fast_strips takes the levels whose cells are at most 32 px wide (16 pixel pairs = one DPP row), k_fast_cells the rest
    for (int l = 0; l <= ORBX_MAX_LEVELS; l++) {
        p.stripBase[l] = p.totalStrips;
        if (l < nl && p.geom[l].wCell <= 32) {
            p.totalStrips += p.geom[l].nRows * ((p.geom[l].nCols + 3) / 4);
            p.stripLevels |= 1u << l;
        }
    }
    p.totalCells = cellBase;
    p.lvlKpCap = lvlKpOff;
    p.pyrImgBytes = (poff + 255) & ~(size_t)255;
    p.slotsPerImg = slotOff;
    p.keysPerImg = (keyOff + 7) & ~(size_t)7;
    p.fastTileStride = (maxTw + 6 + 3) & ~3;        // dwords per pair-tile row (column = byte offset in the aligned row)
    p.fastScoreStride = (maxTw - 6 + 4 + 3) & ~3;   // bytes per score row: 2-px left halo + >= 2 right
    p.fastTileRows = maxTh;
    p.fastLdsPerWave = (4 * p.fastTileStride * maxTh + p.fastScoreStride * (maxTh - 4) + 15) & ~15;
    p.octLdsBytes = oct_exact_lds_bytes(p.maxNodeCap, maxCells);
    if (p.octPyrLdsBytes > ORBX_LDS_LIMIT) { orbx_set_error("quad-tree pyramid needs %zu B of LDS", p.octPyrLdsBytes); return ORBX_ERR_UNSUPPORTED; }
    if (p.octLdsBytes > ORBX_LDS_LIMIT) { orbx_set_error("quad-tree needs %zu B of LDS (features per level %d): unsupported", p.octLdsBytes, p.maxNodeCap); return ORBX_ERR_UNSUPPORTED; }
    *out = std::move(p);
    return ORBX_OK;
}

// ---- k_pyr_level's per-wave set-up, tabulated (orbx_pyramid.hip).  Everything a wave of the level kernel used to derive from the
// resize tables before its first source-row load depends on the image size alone, so it is built here, once per size:
//  * one column record per (level l >= 1, lane slot).  A level has nxc * 64 slots, nxc = ceil((w + 1) / 128): whole waves, so the
//    kernel's 16-byte load needs no clamp.  Slot j owns the columns x0 = 2j - 1 and x0 + 1; the columns -1 and >= w read the
//    nearest inner column (offsets that stay inside the source row) and slots with x0 >= w store nothing.
//  * one band record per (level l >= 1, form RW in {8, 16}, band of RW output rows): the first source row, which source rows an
//    output row is due after, and that row's betas.  The betas are indexed by SOURCE-ROW STEP k (the output row whose second source
//    row is rf + k), not by output row: the kernel's loop over source rows is unrolled, so every beta sits at a FIXED word of the
//    record (lane i of the wave loads word i, a row fetches its word by v_readlane with a constant lane) and no row needs an indexed
//    fetch.  A word is b0 << 12 | b1: one scalar AND gives b0 as v_mul_hi_u32_u24 takes it, an AND and a shift b1.  The table ends
//    with a wave's worth of zero words, so that the lanes past a record's end load inside it too.
// The 16-row records exist only up to scale factor 1.25: beyond it launch_pyramid never picks that form.
struct PyrColRec {          // 16 bytes, one lane's load
    uint32_t A;             // aligned byte offset in the padded source row: both byte pairs lie inside [A, A + 8)
    uint32_t sel;           // oa | ob << 8 | storeValid << 16: byte offsets of the two pairs from A (the v_perm selectors follow)
    uint32_t aa, ab;        // packed (a0, a1) of the two columns
};
#define PYR_BAND_HEAD 8     // words in front of a band record's betas
enum { PYR_BAND_RF = 0, PYR_BAND_MASK = 1, PYR_BAND_LASTK = 2, PYR_BAND_NROW = 3, PYR_BAND_REGULAR = 4, PYR_BAND_DROW = 5, PYR_BAND_SROW = 6 };
static inline int pyr_band_sr(int rw) { return rw == 16 ? 22 : 12; }                         // source rows a band of rw output rows fetches up front
static inline int pyr_band_words(int rw) { return PYR_BAND_HEAD + pyr_band_sr(rw); }   // head, then b0 << 12 | b1 per source-row step
struct PyrRecords {
    std::vector<PyrColRec> cols;
    std::vector<uint32_t> bands;
    int nxc[ORBX_MAX_LEVELS], colOff[ORBX_MAX_LEVELS];           // waves per row band; first column record of the level
    int nbands[2][ORBX_MAX_LEVELS], bandOff[2][ORBX_MAX_LEVELS];   // [0] the 8-row form, [1] the 16-row form: bands; first WORD of the level's records (-1: not built)
};
// floor(2^32 / d) rounded down once more where d is a power of two: udiv_rcp (orbx_pyramid.hip) divides by it with scalar multiplies
static inline uint32_t pyr_rcp(uint32_t d) { return 0xFFFFFFFFu / std::max(d, 1u); }

// Plain C++, no HIP call: reads the SizeInput and the resize tables of the plan.
static inline void plan_pyr_records(const SizeInput &in, const SizePlan &sp, PyrRecords *out) {
    PyrRecords r = {};
    const std::vector<int32_t> &tab = sp.tab;
    for (int l = 0; l < ORBX_MAX_LEVELS; l++) r.bandOff[0][l] = r.bandOff[1][l] = -1;
    for (int l = 1; l < in.nlevels; l++) {
        const LevelGeom &G = sp.geom[l], &S = sp.geom[l - 1];
        const int nxc = (G.w + 1 + 127) / 128;
        r.nxc[l] = nxc;
        r.colOff[l] = (int)r.cols.size();
        for (int j = 0; j < nxc * 64; j++) {
            const int x0 = 2 * j - 1, x1 = x0 + 1;
            const int xa = std::min(std::max(x0, 0), G.w - 1), xb = std::min(x1, G.w - 1);
            const int ca = ORBX_EDGE + tab[G.xofsOff + xa], cb = ORBX_EDGE + tab[G.xofsOff + xb];   // byte column in the padded source row
            PyrColRec c;
            c.A = (uint32_t)(ca & ~3);                  // cb - ca <= 2 (scale factor <= 3)
            c.sel = (uint32_t)(ca - (int)c.A) | ((uint32_t)(cb - (int)c.A) << 8) | (x0 < G.w ? 1u << 16 : 0u);
            c.aa = (uint32_t)tab[G.xalphaOff + xa];
            c.ab = (uint32_t)tab[G.xalphaOff + xb];
            r.cols.push_back(c);
        }
        for (int f = 0; f < 2; f++) {
            const int RW = f ? 16 : 8, SR = pyr_band_sr(RW), words = pyr_band_words(RW);
            if (f == 1 && !(in.scale_factor <= 1.25f)) continue;
            const int nb = (G.h + RW - 1) / RW;
            r.nbands[f][l] = nb;
            r.bandOff[f][l] = (int)r.bands.size();
            r.bands.resize(r.bands.size() + (size_t)nb * words, 0u);
            for (int band = 0; band < nb; band++) {
                uint32_t *w = &r.bands[(size_t)r.bandOff[f][l] + (size_t)band * words];
                const int y0 = band * RW, nrow = std::min(RW, G.h - y0);
                const int rf = tab[G.yofsOff + y0];
                // the rule of the fast path: every row's two source rows exist unclamped, lie within the SR rows fetched up front, and
                // no two output rows share their second source row
                bool regular = rf >= 0;
                uint32_t mask = 0;
                for (int i = 0; i < nrow && regular; i++) {
                    const int sy = tab[G.yofsOff + y0 + i], kk = sy + 1 - rf;
                    regular = sy + 1 <= S.h - 1 && kk < SR && (i == 0 || sy > tab[G.yofsOff + y0 + i - 1]);
                    if (regular) mask |= 1u << kk;
                }
                w[PYR_BAND_RF] = (uint32_t)rf;
                w[PYR_BAND_NROW] = (uint32_t)nrow;
                w[PYR_BAND_DROW] = (uint32_t)((ORBX_EDGE + y0) * G.pstride + ORBX_EDGE - 1);   // byte offset of column -1 of the band's first row in the padded level
                if (!regular) continue;   // the row-by-row path reads the tables itself: the rest of the record stays zero
                w[PYR_BAND_REGULAR] = 1;
                w[PYR_BAND_MASK] = mask;
                int lastk = 0;
                while ((mask >> lastk) > 1u) lastk++;
                w[PYR_BAND_LASTK] = (uint32_t)lastk;
                w[PYR_BAND_SROW] = (uint32_t)(rf * S.pstride);   // byte offset of source row rf from the padded row of source row 0
                for (int i = 0; i < nrow; i++) {
                    const int kk = tab[G.yofsOff + y0 + i] + 1 - rf;
                    const uint32_t bb = (uint32_t)tab[G.ybetaOff + y0 + i];
                    w[PYR_BAND_HEAD + kk] = ((bb & 0xFFFu) << 12) | ((bb >> 16) & 0xFFFu);   // beta <= 2048: 12 bits each
                }
            }
        }
    }
    r.bands.resize(r.bands.size() + 64, 0u);   // lane i of a wave loads word i of its record: whole waves past the last record too
    *out = std::move(r);
}
