// orbx_extract.hip — MI355X (gfx950) ORB front-end: hand-written HIP kernels + C ABI.
//
// Replaces ORBextractor::operator() of kimwin2/ORB_SLAM2v2-1 (reference:
// src/ORBextractor.cc:1043-1105) for batches of equally sized frames:
//   K1 k_pyramid_fused               ComputePyramid, one launch      (:1107-1132)
//   K2 k_fast_cells                  per-cell cv::FAST + fallback   (:789-829)
//   K3 k_octree                      DistributeOctTree              (:539-763)
//   K4 k_describe                    IC_Angle + GaussianBlur + rBRIEF (:77-147, :1085-1090)
// Integer / bitwise work: no MFMA.  Build with -ffp-contract=off (the float expressions of
// the reference are evaluated operation by operation).
#include "orbx_extract_dev.h"
#ifdef ORBX_DEVELOPER
#include "orbx_dev.h"
#include "orbx_dev_pyr.h"
#include "orbx_dev_level0.h"
#endif
#include <math.h>
#include <float.h>
#include <stdarg.h>
#include <algorithm>

// ------------------------------------------------------------------------------------
// error string
static thread_local char g_err[512] = "";
void orbx_set_error(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char *orbx_last_error(void) { return g_err; }
extern "C" const char *orbx_version(void) { return "orbx 0.1 (gfx950)"; }
extern "C" int orbx_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// The matcher entry points keep grow-only device scratch + pinned mirrors + one stream per HOST THREAD (so that they
// are re-entrant without locks).  A thread that is about to exit - or wants its memory back - calls this.
extern "C" int orbx_thread_release_scratch(void) {
    orbx_internal_release_match_scratch();
    orbx_internal_release_arena();
    orbx_internal_release_bow_scratch();
    orbx_internal_release_pose_scratch();
    orbx_internal_release_init_scratch();
    orbx_internal_release_sim3_scratch();
    orbx_internal_release_pnp_scratch();
    orbx_internal_release_sim3opt_scratch();
    orbx_internal_release_newpoints_scratch();
    orbx_internal_release_lba_scratch();
    orbx_internal_release_essential_scratch();
    orbx_internal_release_covis_scratch();
    orbx_internal_release_mapcorrect_scratch();
    return ORBX_OK;
}
#ifdef ORBX_DEVELOPER
// include/orbx_dev.h: the calling thread's three scratch records, read only (no HIP call, nothing allocated)
extern "C" int orbm_debug_thread_scratch(int64_t *out, int n_out) {
    if (!out || n_out != ORBM_DEBUG_THREAD_SCRATCH_INTS) { orbx_set_error("orbm_debug_thread_scratch: bad arguments"); return ORBX_ERR_ARG; }
    orbx_internal_arena_info(out);
    orbx_internal_match_scratch_info(out + 5);
    orbx_internal_bow_scratch_info(out + 7);
    return ORBX_OK;
}

// include/orbx_dev.h: fill every new scratch block (scratch_malloc / scratch_host_malloc, orbx_internal.h).  Process-wide, atomic, off by default
static int g_fillOn = 0;
static uint32_t g_fillWord = 0;
static long long g_fillBlocks = 0, g_fillBytes = 0;
extern "C" int orbx_debug_set_alloc_fill(int enable, uint32_t word) {
    __atomic_store_n(&g_fillOn, 0, __ATOMIC_SEQ_CST);
    __atomic_store_n(&g_fillWord, word, __ATOMIC_SEQ_CST);
    __atomic_store_n(&g_fillBlocks, 0, __ATOMIC_SEQ_CST);
    __atomic_store_n(&g_fillBytes, 0, __ATOMIC_SEQ_CST);
    __atomic_store_n(&g_fillOn, enable ? 1 : 0, __ATOMIC_SEQ_CST);
    return ORBX_OK;
}
extern "C" int orbx_debug_alloc_fill_stats(int64_t out[2]) {
    if (!out) { orbx_set_error("orbx_debug_alloc_fill_stats: bad arguments"); return ORBX_ERR_ARG; }
    out[0] = __atomic_load_n(&g_fillBlocks, __ATOMIC_SEQ_CST);
    out[1] = __atomic_load_n(&g_fillBytes, __ATOMIC_SEQ_CST);
    return ORBX_OK;
}
// a block's bytes are the word's, little endian, repeated: whole words by a 32-bit memset, the up to three bytes behind them one by one
hipError_t orbx_internal_scratch_filled(void *p, size_t bytes, bool pinned) {
    if (!__atomic_load_n(&g_fillOn, __ATOMIC_SEQ_CST) || !p || bytes == 0) return hipSuccess;
    const uint32_t word = __atomic_load_n(&g_fillWord, __ATOMIC_SEQ_CST);
    const size_t nw = bytes / 4;
    if (pinned) {
        for (size_t i = 0; i < nw; i++) ((volatile uint32_t *)p)[i] = word;
        for (size_t i = nw * 4; i < bytes; i++) ((volatile uint8_t *)p)[i] = (uint8_t)(word >> (8 * (i & 3)));
    } else {
        hipError_t e = nw ? hipMemsetD32((hipDeviceptr_t)p, (int)word, nw) : hipSuccess;
        for (size_t i = nw * 4; i < bytes && e == hipSuccess; i++) e = hipMemset((uint8_t *)p + i, (int)((word >> (8 * (i & 3))) & 255u), 1);
        if (e == hipSuccess) e = hipDeviceSynchronize();
        if (e != hipSuccess) return e;
    }
    __atomic_fetch_add(&g_fillBlocks, 1, __ATOMIC_SEQ_CST);
    __atomic_fetch_add(&g_fillBytes, (long long)bytes, __ATOMIC_SEQ_CST);
    return hipSuccess;
}
#endif

// Per-handle options (include/orbx.h): which of several kernels / launch arrangements with identical results the handle uses.
// There is no process-global switch.  Keys 0, 1, 7 stop a kernel after phase n (ablation timing; outputs incomplete) and exist only
// in a developer build (-DORBX_DEVELOPER).
extern "C" int orbx_set_option(orbx_extractor_t *h, int key, int value) {
    static const signed char maxv[ORBX_NUM_OPTIONS] = {/*0*/ -1, -1, -2, 64, 3, 4, 3, -1, ORBX_MAX_CHUNKS, 1, 3, 2, 1, 2, 127, ORBX_MAX_LEVELS,
                                                       /*16*/ 2, -2, 1, ORBX_MAX_LEVELS, 2, 40, 2, 1, 2, 3, 1, 1, -2, -2, -2, -2};
    if (!h || key < 0 || key >= ORBX_NUM_OPTIONS || maxv[key] == -2) { orbx_set_error("orbx_set_option: unknown key %d", key); return ORBX_ERR_ARG; }
#ifdef ORBX_DEVELOPER
    if (maxv[key] == -1) { if (value < 0) return ORBX_ERR_ARG; h->opt[key] = value; return ORBX_OK; }
#else
    if (maxv[key] == -1) { orbx_set_error("orbx_set_option: key %d needs a library built with -DORBX_DEVELOPER", key); return ORBX_ERR_ARG; }
#endif
    if (value < 0 || (key != ORBX_OPT_BLUR_THRESHOLD && value > maxv[key])) { orbx_set_error("orbx_set_option: key %d does not take %d", key, value); return ORBX_ERR_ARG; }
    h->opt[key] = value;
    return ORBX_OK;
}
extern "C" int orbx_get_option(const orbx_extractor_t *h, int key, int *value) {
    if (!h || !value || key < 0 || key >= ORBX_NUM_OPTIONS) return ORBX_ERR_ARG;
    *value = h->opt[key];
    return ORBX_OK;
}

// ------------------------------------------------------------------------------------
// host side
extern "C" int orbx_create(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th,
                           int device, orbx_extractor_t **out) {
    return orbx_create_flavoured(nfeatures, scale_factor, nlevels, ini_th, min_th, device, nullptr, out);
}
extern "C" int orbx_get_flavour(const orbx_extractor_t *h, orbx_flavour_t *out) {
    if (!h || !out) return ORBX_ERR_ARG;
    *out = h->flavour;
    return ORBX_OK;
}
extern "C" int orbx_create_flavoured(int nfeatures, float scale_factor, int nlevels, int ini_th, int min_th,
                                     int device, const orbx_flavour_t *flavour, orbx_extractor_t **out) {
    if (!out) { orbx_set_error("orbx_create: out is NULL"); return ORBX_ERR_ARG; }
    *out = nullptr;
    if (flavour) {
        bool ok = flavour->gauss_rounding == ORBX_GAUSS_ROUND_HALF_UP || flavour->gauss_rounding == ORBX_GAUSS_ROUND_SSE2 ||
                  flavour->gauss_rounding == ORBX_GAUSS_FIXED_TAPS;
        for (int i = 0; i < 3; i++) ok = ok && flavour->reserved[i] == 0;
        const int32_t *k = flavour->gauss_taps;
        if (flavour->gauss_rounding == ORBX_GAUSS_FIXED_TAPS) {   // Q8 taps, centre first; a row sum (<= 255 * their sum) must fit 16 bits
            for (int i = 0; i < 4; i++) ok = ok && k[i] >= 0 && k[i] <= 255;
            ok = ok && k[0] >= 1 && k[0] + 2 * (k[1] + k[2] + k[3]) <= 257;
        } else
            for (int i = 0; i < 4; i++) ok = ok && k[i] == 0;
        if (!ok) {
            orbx_set_error("orbx_create_flavoured: unknown flavour (gauss_rounding=%d, gauss_taps=%d %d %d %d)", flavour->gauss_rounding, k[0], k[1], k[2], k[3]);
            return ORBX_ERR_ARG;
        }
    }
    if (nfeatures < 1 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !(scale_factor > 1.0f) || ini_th < 0 ||
        min_th < 0 || ini_th > 255 || min_th > 255) {
        orbx_set_error("orbx_create: bad arguments (nfeatures=%d scale=%f nlevels=%d ini=%d min=%d)", nfeatures,
                       scale_factor, nlevels, ini_th, min_th);
        return ORBX_ERR_ARG;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0 || device < 0 || device >= ndev) {
        orbx_set_error("orbx_create: no usable HIP device (count=%d, requested %d): %s", ndev, device,
                       e == hipSuccess ? "ok" : hipGetErrorString(e));
        return ORBX_ERR_NO_DEVICE;
    }
    ORBX_HIP(hipSetDevice(device));
    orbx_extractor *h = new orbx_extractor();   // (value-initialised: every field 0)
    h->nfeatures = nfeatures; h->nlevels = nlevels; h->ini_th = ini_th; h->min_th = min_th;
    h->device = device; h->scale_factor = scale_factor;
    if (flavour) h->flavour = *flavour;
    extractor_tables(nfeatures, h->scale_factor, nlevels, &h->tb);
    ORBX_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    // host-mapped word the quad-tree kernels store a call's sequence number into when they flag a corner-sparse level (launch_chunk)
    ORBX_HIP(scratch_host_malloc((void **)&h->h_sparseSeen, sizeof(int32_t), hipHostMallocMapped | hipHostMallocCoherent));
    *h->h_sparseSeen = (int32_t)0xC0000000u;   // far behind call 0 in unsigned distance
    ORBX_HIP(hipHostGetDevicePointer((void **)&h->d_sparseSeen, h->h_sparseSeen, 0));
    for (int i = 0; i < ORBX_SIDE_STREAMS; i++) {
        ORBX_HIP(hipStreamCreateWithFlags(&h->side[i], hipStreamNonBlocking));
        ORBX_HIP(hipEventCreateWithFlags(&h->evJoin[i], hipEventDisableTiming));
    }
    for (int i = 0; i < ORBX_MAX_CHUNKS; i++) ORBX_HIP(hipEventCreateWithFlags(&h->evPyr[i], hipEventDisableTiming));
    // evFastDone orders the side stream's kernels behind FAST for SPEED only (they touch nothing FAST reads or writes): no memory fence
    // is needed when it fires.
    ORBX_HIP(hipEventCreateWithFlags(&h->evFastDone, hipEventDisableTiming | hipEventDisableSystemFence));
    ORBX_HIP(hipEventCreateWithFlags(&h->evGather, hipEventDisableTiming));
    ORBX_HIP(hipEventCreateWithFlags(&h->evOctA, hipEventDisableTiming));
    ORBX_HIP(hipEventCreateWithFlags(&h->evPrefetch, hipEventDisableTiming | hipEventDisableSystemFence));   // consumer: a kernel of the same device
    for (int r = 0; r < ORBX_EV_RING; r++)
        // timing-only events: no system-scope fence (cache write-back + invalidate) when they complete — with the default
        // flags every stage boundary of a profiled batch cost ~5 us of idle GPU, which the step time then contained
        for (int i = 0; i < ORBX_NUM_STAGES; i++) ORBX_HIP(hipEventCreateWithFlags(&h->ev[r][i], hipEventDisableSystemFence));
    *out = h;
    return ORBX_OK;
}

// The size-dependent device buffers of a plan for batches of B images: {the handle's pointer, bytes, zero-filled?}.  ensure_plan
// allocates from this list and free_plan frees by it.
struct PlanBuffer { void **ptr; size_t bytes; bool zero; };
static std::vector<PlanBuffer> plan_buffers(orbx_extractor *h, const SizePlan &sp, int B) {
    const size_t Bz = (size_t)B, lv = (size_t)ORBX_MAX_LEVELS * Bz, slots = Bz * h->nlevels;
    const size_t hist = (size_t)ORBX_HIST_IMAGES * h->nlevels * sp.histStride;   // small batches: 4 image slots (FastHist)
    std::vector<PlanBuffer> v = {
        {(void **)&h->d_geom, sizeof(LevelGeom) * ORBX_MAX_LEVELS, false},
        {(void **)&h->d_tab, sizeof(int32_t) * std::max<size_t>(sp.tab.size(), 1), false},
        {(void **)&h->d_pyr, sp.pyrImgBytes * Bz, false},
        {(void **)&h->d_cellCnt, sizeof(uint32_t) * sp.totalCells * Bz, false},
        {(void **)&h->d_cellRaw, sizeof(uint32_t) * sp.totalCells * Bz, false},
        {(void **)&h->d_slots, sizeof(uint32_t) * (sp.slotsPerImg * Bz + 64), false},   // + 64: the 16-byte list reads of k_octree_pyr may run past the last cell's block
        {(void **)&h->d_cand, sizeof(uint32_t) * sp.keysPerImg * Bz, false},
        {(void **)&h->d_nodeOf, sizeof(uint16_t) * sp.keysPerImg * Bz, false},
        {(void **)&h->d_candCnt, sizeof(int32_t) * lv, false},
        {(void **)&h->d_lvlCnt, sizeof(int32_t) * lv, false},
        {(void **)&h->d_sparse, sizeof(int32_t) * lv, true},   // first call: every level scored row by row
        {(void **)&h->d_lvlKp, sizeof(uint32_t) * (size_t)sp.lvlKpCap * Bz, false},
        {(void **)&h->d_octFallback, sizeof(int32_t) * lv, true},
        {(void **)&h->d_histCnt, sizeof(uint32_t) * hist, true},
        {(void **)&h->d_histBest, sizeof(uint32_t) * hist, true},
        {(void **)&h->d_octPart, sizeof(uint32_t) * slots * OCT_BIG_K * (size_t)sp.octDeepMax, false},
        {(void **)&h->d_octLeaf, sizeof(uint32_t) * slots * (size_t)sp.octPyrWords, false},
        {(void **)&h->d_octBest, sizeof(uint32_t) * slots * (size_t)sp.maxNodeCap, false},
        {(void **)&h->d_octState, sizeof(int32_t) * slots * 4, true},
        {(void **)&h->d_pyrCols, sizeof(PyrColRec) * std::max<size_t>(h->pr.cols.size(), 1), false},
        {(void **)&h->d_pyrBands, sizeof(uint32_t) * std::max<size_t>(h->pr.bands.size(), 1), false},
    };
    if (sp.octSliceStride > 0) {   // shared sweeps of large levels in a batch (OctSrc::nslice): best-key partials beside the count partials of d_octPart, arrival counters
        v.push_back({(void **)&h->d_octPartBest, sizeof(uint32_t) * slots * OCT_MAX_SLICES * (size_t)sp.octSliceStride, false});
        v.push_back({(void **)&h->d_octPartCnt, sizeof(uint32_t) * slots * OCT_MAX_SLICES * (size_t)sp.octSliceStride, false});
        v.push_back({(void **)&h->d_octSliceState, sizeof(int32_t) * slots, true});
    }
    return v;
}

static void free_plan(orbx_extractor *h) {
    for (const PlanBuffer &b : plan_buffers(h, h->sp, h->pB)) { hipFree(*b.ptr); *b.ptr = nullptr; }
    // allocated on first use, with the plan's geometry
    hipFree(h->d_pyrAlt); h->d_pyrAlt = nullptr; h->pyrAltBytes = 0; h->pfValid = 0; h->prevPyrValid = 0;
    hipFree(h->d_pyrNext); h->d_pyrNext = nullptr; h->pyrNextBytes = 0;
    hipFree(h->d_blur); hipFree(h->d_blurAlt); h->d_blur = h->d_blurAlt = nullptr; h->blurBytes = h->blurAltBytes = 0; h->blurMaskLast = h->blurMaskAlt = 0;
    h->sp = SizePlan();
    h->pr = PyrRecords();
    h->pw = h->ph = h->pB = 0;
}

extern "C" int orbx_destroy(orbx_extractor_t *h) {
    if (!h) return ORBX_OK;
    hipSetDevice(h->device);
    hipStreamSynchronize(h->stream);
    if (h->last_valid) hipStreamSynchronize(h->last_stream);
    if (h->st_stream) hipStreamSynchronize(h->st_stream);
    orbx_internal_free_stereo_scratch(h);
    orbx_internal_free_rgbd_scratch(h);
    orbx_internal_free_rect_scratch(h);
    free_plan(h);
    hipFree(h->d_in); hipFree(h->d_kps); hipFree(h->d_desc); hipFree(h->d_counts); hipFree(h->d_dbgBlur);
    hipFree(h->d_sfr); if (h->h_sfr) hipHostFree(h->h_sfr);
    for (int i = 0; i < 2; i++) { hipFree(h->fv_d[i]); if (h->fv_h[i]) hipHostFree(h->fv_h[i]); }
    if (h->fv_stage) hipHostFree(h->fv_stage);
    if (h->fv_flag) hipHostFree(h->fv_flag);
    if (h->h_sparseSeen) hipHostFree(h->h_sparseSeen);
    if (h->h_kps) { hipHostFree(h->h_kps); hipHostFree(h->h_desc); hipHostFree(h->h_counts); }
    for (int r = 0; r < ORBX_EV_RING; r++)
        for (int i = 0; i < ORBX_NUM_STAGES; i++) hipEventDestroy(h->ev[r][i]);
    for (int i = 0; i < ORBX_SIDE_STREAMS; i++) { hipStreamSynchronize(h->side[i]); hipStreamDestroy(h->side[i]); hipEventDestroy(h->evJoin[i]); }
    for (int i = 0; i < ORBX_MAX_CHUNKS; i++) hipEventDestroy(h->evPyr[i]);
    hipEventDestroy(h->evFastDone); hipEventDestroy(h->evPrefetch); hipEventDestroy(h->evGather); hipEventDestroy(h->evOctA);
    hipFree(h->d_kpsB); hipFree(h->d_descB);
    hipStreamDestroy(h->stream);
    delete h;
    return ORBX_OK;
}

extern "C" int orbx_get_levels(const orbx_extractor_t *h) { return h ? h->nlevels : ORBX_ERR_ARG; }
extern "C" float orbx_get_scale_factor(const orbx_extractor_t *h) { return h ? (float)h->scale_factor : 0.f; }
extern "C" int orbx_get_tables(const orbx_extractor_t *h, float *sf, float *isf, float *s2, float *is2,
                               int32_t *nf, int32_t *umax16) {
    if (!h) return ORBX_ERR_ARG;
    for (int i = 0; i < h->nlevels; i++) {
        if (sf) sf[i] = h->tb.sf[i];
        if (isf) isf[i] = h->tb.isf[i];
        if (s2) s2[i] = h->tb.sig2[i];
        if (is2) is2[i] = h->tb.isig2[i];
        if (nf) nf[i] = h->tb.nfeat[i];
    }
    if (umax16) memcpy(umax16, h->tb.umax, sizeof(int32_t) * 16);
    return ORBX_OK;
}
extern "C" int orbx_max_keypoints(const orbx_extractor_t *h) {
    if (!h) return ORBX_ERR_ARG;
    // every level returns at most max(N+2, 4*nIni) nodes; nIni is image dependent (<= 64)
    return h->sp.max_kp > 0 ? h->sp.max_kp : h->nfeatures + 3 * h->nlevels;
}

// The size-dependent plan of the handle: plan_size (orbx_size_plan.h) decides everything - a refused size returns here, with the
// handle's current plan and buffers untouched - then the buffers of plan_buffers are replaced and geom / tab uploaded.
static int ensure_plan(orbx_extractor *h, int w, int hgt, int B) {
    if (h->pw == w && h->ph == hgt && h->pB >= B) return ORBX_OK;
    SizePlan sp;
    const SizeInput in = {w, hgt, h->nlevels, h->scale_factor, h->tb, h->opt[3]};
    const int rc = plan_size(in, &sp);
    if (rc) return rc;
    PyrRecords pr;
    plan_pyr_records(in, sp, &pr);
    ORBX_HIP(hipSetDevice(h->device));
    if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
    for (int i = 0; i < ORBX_SIDE_STREAMS; i++) ORBX_HIP(hipStreamSynchronize(h->side[i]));
    if (h->pw == w && h->ph == hgt) B = std::max(B, h->pB);   // (an unchanged size keeps the larger capacity)
    free_plan(h);
    h->sp = std::move(sp);
    h->pr = std::move(pr);
    for (const PlanBuffer &b : plan_buffers(h, h->sp, B)) {
        ORBX_HIP(scratch_malloc(b.ptr, b.bytes));
        if (b.zero) ORBX_HIP(hipMemset(*b.ptr, 0, b.bytes));
    }
    ORBX_HIP(hipMemcpy(h->d_geom, h->sp.geom, sizeof(LevelGeom) * ORBX_MAX_LEVELS, hipMemcpyHostToDevice));
    if (!h->sp.tab.empty()) ORBX_HIP(hipMemcpy(h->d_tab, h->sp.tab.data(), sizeof(int32_t) * h->sp.tab.size(), hipMemcpyHostToDevice));
    if (!h->pr.cols.empty()) ORBX_HIP(hipMemcpy(h->d_pyrCols, h->pr.cols.data(), sizeof(PyrColRec) * h->pr.cols.size(), hipMemcpyHostToDevice));
    if (!h->pr.bands.empty()) ORBX_HIP(hipMemcpy(h->d_pyrBands, h->pr.bands.data(), sizeof(uint32_t) * h->pr.bands.size(), hipMemcpyHostToDevice));
    h->pw = w; h->ph = hgt; h->pB = B;
    return ORBX_OK;
}

// add the finished event set `slot` to the per-stage accumulators
static int harvest_events(orbx_extractor *h, int slot) {
    hipEvent_t *ev = h->ev[slot];
    if (h->ev_pending[slot] == 2) {   // mode 2: only the FAST kernel was bracketed
        float ms = 0;
        ORBX_HIP(hipEventSynchronize(ev[2]));
        ORBX_HIP(hipEventElapsedTime(&ms, ev[1], ev[2]));
        h->acc_ms[1] += ms;
        h->acc_n++;
        h->ev_pending[slot] = 0;
        return ORBX_OK;
    }
    ORBX_HIP(hipEventSynchronize(ev[4]));
    for (int i = 0; i < 4; i++) {
        float ms = 0;
        ORBX_HIP(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        h->acc_ms[i] += ms;
    }
    float tot = 0;
    ORBX_HIP(hipEventElapsedTime(&tot, ev[0], ev[4]));
    h->acc_ms[4] += tot;
    h->acc_n++;
    h->ev_pending[slot] = 0;
    return ORBX_OK;
}

__global__ void k_nop() {}

// Which levels are blurred as a whole (k_blur_levels) instead of per keypoint inside k_describe, and their tiles.  A level of P_l
// pixels with a budget of N_l keypoints costs N_l * 43 * 40 blurred pixels per keypoint block in the fused form; the level-wide
// form costs P_l once plus a second staging load per keypoint.  Rule: N_l * 37^2 * 100 >= thr * P_l (developer knob 14 = thr in
// percent; knob 13: 1 = never, 2 = every level).  Results are identical either way.
// MEASURED (round 3, MI355X): the level-wide form LOSES at every size tried, so the default threshold is out of reach and the
// form stays a tested alternative.  64 stereo frames 1241x376: 1000 features 0.650 ms per step with no level blurred as a whole,
// 0.694 with the rule at 120 %, 0.901 with every level; 2000 features 0.858 / 1.047 / 1.047; 32 images 1920x1080 / 4000 features
// 0.736 / 0.724 / 0.925.  Alone on the GPU at 2000 features: k_describe 0.325 -> 0.19 ms (its staging grows from 9 to 12 loads per
// lane, which is what it is bound by once the blur passes are gone), k_blur_levels 0.26 ms (its row loop serialises on the
// reflected-border branches; a branch-free version would still move 2.4 bytes per pixel: ~0.08 ms), so even the best case wins
// ~0.05 of 0.89 ms at 2000 features and nothing at 1000.
#define ORBX_BLUR_THR 100000000
static unsigned blur_plan(const orbx_extractor *h, BlurPlan &bp, int &totalTiles) {
    unsigned mask = 0;
    totalTiles = 0;
    const long thr = h->opt[14] > 0 ? h->opt[14] : ORBX_BLUR_THR;
    for (int l = 0; l <= ORBX_MAX_LEVELS; l++) {
        bp.tileBase[l] = totalTiles;
        if (l >= h->nlevels) continue;
        const LevelGeom &g = h->sp.geom[l];
        const bool on = h->opt[13] == 2 || (h->opt[13] == 0 && (long)g.N * 1369 * 100 >= thr * (long)g.w * g.h);
        bp.tilesX[l] = 0;
        if (!on) continue;
        mask |= 1u << l;
        const int ndw = ((g.w + ORBX_EDGE - 1) >> 2) - 4 + 1;
        bp.tilesX[l] = (ndw + 63) / 64;
        totalTiles += bp.tilesX[l] * ((g.h + BLUR_R - 1) / BLUR_R);
    }
    return mask;
}
// the Gaussian's taps as the kernels take them: k3 | k2 << 8 | k1 << 16 | k0 << 24 (orbx_flavour_t lists the centre first)
static uint32_t gauss_taps_packed(const orbx_extractor *h) {
    if (h->flavour.gauss_rounding != ORBX_GAUSS_FIXED_TAPS) return ORBX_GAUSS_TAPS_DEFAULT;
    const int32_t *k = h->flavour.gauss_taps;
    return (uint32_t)k[3] | ((uint32_t)k[2] << 8) | ((uint32_t)k[1] << 16) | ((uint32_t)k[0] << 24);
}
static int ensure_blur(orbx_extractor *h, uint8_t **buf, size_t *bytes) {
    const size_t need = h->sp.pyrImgBytes * (size_t)h->pB;
    if (*bytes >= need) return ORBX_OK;
    if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
    for (int i = 0; i < ORBX_SIDE_STREAMS; i++) ORBX_HIP(hipStreamSynchronize(h->side[i]));
    hipFree(*buf); *buf = nullptr; *bytes = 0;
    ORBX_HIP(scratch_malloc(buf, need));
    *bytes = need;
    return ORBX_OK;
}
// the level-wide blur behind a pyramid (same stream); returns the mask of blurred levels through *maskOut
static int launch_blur(orbx_extractor *h, const uint8_t *pyr, uint8_t **blurBuf, size_t *blurBytes, int b0, int B, hipStream_t st, unsigned *maskOut) {
    BlurPlan bp;
    int tiles = 0;
    const unsigned mask = blur_plan(h, bp, tiles);
    *maskOut = mask;
    if (!mask) return ORBX_OK;
    int rc = ensure_blur(h, blurBuf, blurBytes);
    if (rc) return rc;
    const size_t off = (size_t)b0 * h->sp.pyrImgBytes;   // images [b0, b0 + B) of both buffers
    hipLaunchKernelGGL(k_blur_levels, dim3((tiles + 3) / 4, B), dim3(256), 0, st, pyr + off, *blurBuf + off, h->sp.pyrImgBytes, h->d_geom, h->nlevels, tiles, bp,
                       h->flavour.gauss_rounding, gauss_taps_packed(h));
    return ORBX_OK;
}

// K1: ComputePyramid of B images into pyr.  Developer knob 5: 0 / 2 = one launch per level (the default), 1 = every level in the
// fused launch, 3 = hybrid.
static bool pyramid_fused_all(const orbx_extractor *h) { return h->opt[5] == 1 || h->scale_factor > 3.0; }
// Level 0 of a batch: the copy of the input into the padded level (with its REFLECT_101 frame).
static void launch_pad0(orbx_extractor *h, const uint8_t *d_imgs, uint8_t *pyr, int B, int stride, size_t img_stride, hipStream_t st) {
    const LevelGeom &g0 = h->sp.geom[0];
    // level 0 of a small batch: source rows staged in LDS (ORBX_OPT_PAD_FORM: 0 = by batch size, 1 = never, 2 = always) - the image of a latency
    // call is read in pinned host memory, where each byte should cross the bus once, in aligned transactions
    const size_t padLds = (size_t)PAD_ROWS_PER_BLOCK * stride + 32;
    if ((h->opt[24] == 2 || (h->opt[24] == 0 && B <= ORBX_HIST_IMAGES)) && padLds <= 60 * 1024)
        hipLaunchKernelGGL(k_pyr_pad_rows, dim3((g0.h + PAD_ROWS_PER_BLOCK - 1) / PAD_ROWS_PER_BLOCK, B), dim3(256), padLds, st, d_imgs, stride, img_stride, pyr,
                           h->sp.pyrImgBytes, h->d_geom);
    else {
        // the interior 16-byte chunks of PAD_FULL_ROWS padded rows per blockIdx.y (whole waves, at most 256 threads), then the rows of
        // blocks that share out the chunks touching the frame (the kernel derives the same nI / nE / rowBlocks from the level's geometry)
        const int pc = g0.pstride >> 4, cI0 = (ORBX_EDGE + 15) >> 4, cI1 = std::max((g0.w + ORBX_EDGE) >> 4, cI0), nI = cI1 - cI0, nE = pc - nI;
        const int threads = std::min(256, std::max(64, (nI + 63) & ~63)), gx = std::max(1, (nI + threads - 1) / threads);
        const int rowBlocks = (g0.prows + PAD_FULL_ROWS - 1) / PAD_FULL_ROWS, edgeRows = (nE * g0.prows + gx * threads - 1) / (gx * threads);
        hipLaunchKernelGGL(k_pyr_pad<true>, dim3(gx, rowBlocks + edgeRows, B), dim3(threads), 0, st, d_imgs, stride, img_stride, pyr,
                           h->sp.pyrImgBytes, h->d_geom, 0);
    }
}
// In-place input (orbx_extract_batch_device_padded) is taken when nothing of the call wants level 0 inside the pyramid block: not the
// level-wide blur of level 0 (k_blur_levels reads the frame), not the forms of a latency call (B <= ORBX_HIST_IMAGES: level chains and
// the LDS-staged copy, which start from the pyramid block), not a developer knob that picks another pyramid form.  Otherwise the call
// copies level 0 as a dense call does - same results, and orbx_debug_level0_in_place tells which it was.
// The pyramid is launched per CHUNK (ORBX_OPT_CHUNKS; launch_pipeline cuts the call, launch_pyramid picks its forms from the chunk's
// images), so the batch size that counts is the smallest chunk's: nch = the chunks the call's pyramid launches are cut into (1 for a
// pyramid built ahead, which is one launch of the whole batch).
static bool level0_in_place_ok(const orbx_extractor *h, int B, int nch) {
    BlurPlan bp;
    int tiles = 0;
    if (blur_plan(h, bp, tiles) & 1u) return false;
    const int smallest = B / std::max(nch, 1);   // launch_pipeline: chunk c gets (B - b0) / (nch - c) images, the first one the fewest
    return smallest > ORBX_HIST_IMAGES && !pyramid_fused_all(h) && (h->opt[5] == 0 || h->opt[5] == 2) && h->opt[24] != 2;
}
// lv0.base != NULL: level 0 stays where it is (the caller's images, in the padded level's layout); level 1 is resized from there.
static void launch_pyramid(orbx_extractor *h, const uint8_t *d_imgs, uint8_t *pyr, int B, int stride, size_t img_stride, hipStream_t st, const Level0 &lv0) {
    const int nl = h->nlevels;
    if (pyramid_fused_all(h)) {   // writes every frame itself (a lane's two source byte pairs fit 8 bytes only up to scale 3)
        hipLaunchKernelGGL(k_pyramid_fused, dim3(h->sp.pyrTilesX * h->sp.pyrTilesY, B), dim3(256), h->sp.pyrLdsBytes, st, d_imgs,
                           stride, img_stride, pyr, h->sp.pyrImgBytes, h->d_geom, nl, h->d_tab, h->sp.pyrXSpanOff,
                           h->sp.pyrYSpanOff, h->sp.pyrTilesX, h->sp.pyrTilesY, h->sp.pyrBufBytes, h->sp.pyrMaxPar, 0);
        return;
    }
    // Hybrid form (developer knob 5 = 3, parity-tested, NOT used by default): levels 1, 2 one launch each, levels 3.. from ONE launch
    // that chains them through LDS - VERDICT r01's proposal for the launch-latency-bound small levels.  Measured: one 1241x376
    // image 193 us per orbx_extract call against 184 us with seven launches (the chain's five barriers and its generic per-pixel
    // indexing cost more than five ~4-us launches), and for a batch it spends five times the instructions per pixel while the
    // pyramid runs beside VALU-bound kernels.
    const bool hybrid = h->opt[5] == 3;
    const int lastSingle = hybrid ? std::min(2, nl - 1) : nl - 1;
    if (!lv0.base) launch_pad0(h, d_imgs, pyr, B, stride, img_stride, st);
    // ORBX_OPT_PYRAMID_FORM = 4 (and small batches by default, ORBX_OPT_PYR_CHAINS): the levels in chains, one launch per chain
    const int cv = h->opt[25] == 3 ? 1 : 0;   // ORBX_OPT_PYR_CHAINS: 2 / 3 = chains of up to 4 / 7 levels (0: the default, 1: never)
    if (h->sp.nChains[cv] > 0 && !hybrid && (h->opt[5] == 4 || (h->opt[5] == 0 && h->opt[25] != 1 && B <= ORBX_HIST_IMAGES))) {
        for (int c = 0; c < h->sp.nChains[cv]; c++) {
            const ChainPlan &cp = h->sp.chains[cv][c];
            const size_t lds = 2 * (size_t)cp.bufBytes + (size_t)(cp.lb - cp.la) * cp.maxRows * 8;
            hipLaunchKernelGGL(k_pyr_chain, dim3(cp.tilesX * cp.tilesY, B), dim3(256), lds, st, pyr, h->sp.pyrImgBytes, h->d_geom, h->d_tab, cp);
        }
        return;
    }
    for (int l = 1; l <= lastSingle; l++) {
        // 16 output rows per wave while that still leaves every SIMD several waves (8192 = 8 per SIMD), else 8; same pixels either way
        const int nxc = (h->sp.geom[l].w + 1 + 127) / 128, nb16 = (h->sp.geom[l].h + 15) / 16, nb8 = (h->sp.geom[l].h + 7) / 8;
        const bool tall = h->scale_factor <= 1.25f && (h->opt[22] == 0 ? (size_t)nxc * nb16 * B >= 8192 : h->opt[22] == 2);   // (beyond 1.25 the 16-row form cannot cover a band from 22 source rows)
        // the wave's set-up comes from the records of the planned size (plan_pyr_records): the level's column records, the form's band
        // records, and the reciprocals with which the kernel divides by the chunk count and by the grid width on the scalar unit
        const PyrColRec *cols = h->d_pyrCols + h->pr.colOff[l];
        const int f = tall ? 1 : 0, nb = tall ? nb16 : nb8, gx = (nxc * nb + 3) / 4;
        const uint32_t *bands = h->d_pyrBands + h->pr.bandOff[f][l];
        if (tall)
            hipLaunchKernelGGL((k_pyr_level<16, 22>), dim3(gx, B), dim3(256), 0, st, pyr, h->sp.pyrImgBytes, h->d_geom, l, h->d_tab, nxc, nb, cols, bands,
                               pyr_rcp((uint32_t)nxc), pyr_rcp((uint32_t)gx), lv0);
        else
            hipLaunchKernelGGL((k_pyr_level<8, 12>), dim3(gx, B), dim3(256), 0, st, pyr, h->sp.pyrImgBytes, h->d_geom, l, h->d_tab, nxc, nb, cols, bands,
                               pyr_rcp((uint32_t)nxc), pyr_rcp((uint32_t)gx), lv0);
    }
    if (lastSingle < nl - 1)
        hipLaunchKernelGGL(k_pyramid_fused, dim3(h->sp.pyrTilesX * h->sp.pyrTilesY, B), dim3(256), h->sp.pyrLdsBytes, st, d_imgs,
                           stride, img_stride, pyr, h->sp.pyrImgBytes, h->d_geom, nl, h->d_tab, h->sp.pyrXSpanOff,
                           h->sp.pyrYSpanOff, h->sp.pyrTilesX, h->sp.pyrTilesY, h->sp.pyrBufBytes, h->sp.pyrMaxPar, lastSingle);
}

// The per-image buffers of a handle as seen by ONE chunk of a batch: every base pointer already points at the chunk's first image.
struct ChunkView {
    const uint8_t *imgs; uint8_t *pyr; uint32_t *cellCnt, *cellRaw, *slots, *cand, *lvlKp; uint16_t *nodeOf;
    int32_t *candCnt, *lvlCnt, *octFallback, *sparse; orbx_keypoint_t *kps; uint8_t *desc; int32_t *counts;
    int b0;            // first image of the chunk
    Level0 lv0;        // level 0 read in place (base != NULL): the chunk's first image in the caller's buffer
    size_t octSlot0;   // first (image, level) slot of the chunk in the multi-workgroup quad-tree scratch (d_octPart / Leaf / Best / State)
};
static ChunkView chunk_view(const orbx_extractor *h, const uint8_t *d_imgs, size_t img_stride, orbx_keypoint_t *d_kps, uint8_t *d_desc,
                            int32_t *d_counts, int cap, int b0) {
    ChunkView v;
    const size_t z = (size_t)b0;
    v.imgs = d_imgs + z * img_stride; v.pyr = h->d_pyr + z * h->sp.pyrImgBytes;
    v.cellCnt = h->d_cellCnt + z * h->sp.totalCells; v.cellRaw = h->d_cellRaw + z * h->sp.totalCells;
    v.slots = h->d_slots + z * h->sp.slotsPerImg; v.cand = h->d_cand + z * h->sp.keysPerImg; v.nodeOf = h->d_nodeOf + z * h->sp.keysPerImg;
    v.lvlKp = h->d_lvlKp + z * h->sp.lvlKpCap;
    v.sparse = h->d_sparse + z * h->nlevels;
    v.candCnt = h->d_candCnt + z * h->nlevels; v.lvlCnt = h->d_lvlCnt + z * h->nlevels; v.octFallback = h->d_octFallback + z * h->nlevels;
    v.kps = d_kps + z * cap; v.desc = d_desc + z * cap * 32; v.counts = d_counts + b0;
    v.octSlot0 = z * h->nlevels; v.b0 = b0;
    v.lv0 = h->lv0;
    if (v.lv0.base) v.lv0.base += z * v.lv0.imgBytes;
    return v;
}

// What plan_chunk reads, taken from the handle: a chunk of B images of a call cut into nch chunks.
static PlanInput plan_input(const orbx_extractor *h, int B, int nch, bool prof, bool profFast, bool skipPyr, bool evPyrDone) {
    PlanInput in = {};
    in.B = B; in.nl = h->nlevels; in.totalStrips = h->sp.totalStrips; in.stripLevels = (int32_t)h->sp.stripLevels; in.octBigMask = (int32_t)h->sp.octBigMask;
    in.lastChunks = nch; in.prof = prof; in.profFast = profFast; in.skipPyr = skipPyr; in.pfUsed = h->pfUsed != 0; in.evPyrDone = evPyrDone;
    in.dbgBlur = h->d_dbgBlur != nullptr; in.sliceScratch = h->d_octPartBest != nullptr;
    in.fastTileStride = h->sp.fastTileStride; in.fastScoreStride = h->sp.fastScoreStride;
    // the quad-tree of image slot 0 stores the call's sequence number into a host-mapped word when it flags a corner-sparse level
    in.sparseRecent = h->h_sparseSeen && (uint32_t)h->callSeq - (uint32_t)*(volatile int32_t *)h->h_sparseSeen <= 16u;   // (sequence numbers wrap: unsigned distance)
    for (int l = 0; l < h->nlevels; l++) in.ncells[l] = h->sp.geom[l].ncells;
    memcpy(in.opt, h->opt, sizeof(in.opt));
    return in;
}

// the quad-tree kernels in their 512- or 1024-thread build (ChunkPlan::wideOct), on STREAM
#define ORBX_OCT_LAUNCH_ON(STREAM, KERN, KERNW, GRID, LDS, ...)                                                         \
    do {                                                                                                                \
        if (p.wideOct) {                                                                                                \
            ORBX_HIP(hipFuncSetAttribute((const void *)KERNW, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS))); \
            hipLaunchKernelGGL(KERNW, GRID, dim3(OCT_T_WIDE), LDS, STREAM, __VA_ARGS__);                                \
        } else {                                                                                                        \
            ORBX_HIP(hipFuncSetAttribute((const void *)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS)));  \
            hipLaunchKernelGGL(KERN, GRID, dim3(OCT_T), LDS, STREAM, __VA_ARGS__);                                      \
        }                                                                                                               \
    } while (0)
// k_octree_pyr of the levels [LV0, LV0 + grid.y): its arguments but for the phase-stop knobs, the first level and the key source
#define ORBX_OCT_PYR_ON(STREAM, GRID, STOP, PHASE, LV0, SRC)                                                                        \
    ORBX_OCT_LAUNCH_ON(STREAM, k_octree_pyr, k_octree_pyr_wide, GRID, ldsOct, h->d_geom, nl, v.cand, h->sp.keysPerImg, v.candCnt, v.lvlKp, \
                       h->sp.lvlKpCap, v.lvlCnt, h->d_tab, h->sp.maxNodeCap, pow2, h->sp.octPyrWords, v.octFallback, STOP, v.nodeOf, scratch,   \
                       PHASE, 0u, LV0, SRC)
// k_fast_cells: the instance of the plan's compile-time tile stride, with (SP) or without the compaction queue
#define ORBX_LAUNCH_FAST(EST, SP, LDSW)                                                                                  \
    hipLaunchKernelGGL((k_fast_cells<EST, SP>), dim3((h->sp.totalCells + FAST_WAVES - 1) / FAST_WAVES, B), dim3(64 * FAST_WAVES), \
                       (size_t)(LDSW) * FAST_WAVES, st, v.pyr, h->sp.pyrImgBytes, h->d_geom, nl, h->sp.totalCells, v.cellCnt, v.cellRaw, v.slots, \
                       h->sp.slotsPerImg, h->ini_th, h->min_th, h->sp.fastTileStride, h->sp.fastScoreStride, h->sp.fastTileRows, \
                       (LDSW), p.fastPhase, cb, (unsigned)p.stripLevels, v.sparse, (SP) ? FastHist{} : fhist, v.lv0)
#define ORBX_LAUNCH_FAST_ES(SP, LDSW)                         \
    switch (p.es) {                                           \
    case 44: ORBX_LAUNCH_FAST(44, SP, LDSW); break;           \
    case 48: ORBX_LAUNCH_FAST(48, SP, LDSW); break;           \
    case 52: ORBX_LAUNCH_FAST(52, SP, LDSW); break;           \
    default: ORBX_LAUNCH_FAST(0, SP, LDSW); break;            \
    }

// One chunk (B images from v) through the whole pipeline on stream st.  ev / prof / profFast: this chunk carries the stage events;
// evPyrDone (may be NULL) is recorded behind the chunk's pyramid.  Every decision is plan_chunk's (orbx_plan.h): this function reads
// no option, it executes the plan.
static int launch_chunk(orbx_extractor *h, const ChunkView &v, int B, int stride, size_t img_stride, int cap, hipStream_t st,
                        hipEvent_t *ev, bool prof, bool profFast, hipEvent_t evPyrDone, bool skipPyr) {
    ChunkPlan p;
    int rc = plan_chunk(plan_input(h, B, h->lastChunks, prof, profFast, skipPyr, evPyrDone != nullptr), &p);
    if (rc) return rc;   // (a plan that breaks an invariant of the kernels launches nothing)
    if (v.b0 == 0) h->lastPlan = p;
    const int nl = h->nlevels;
    CellBases cb;
    for (int l = 0; l <= ORBX_MAX_LEVELS; l++) cb.v[l] = l < nl ? h->sp.geom[l].cellBase : h->sp.totalCells;
    StripBases sb;
    for (int l = 0; l <= ORBX_MAX_LEVELS; l++) sb.v[l] = h->sp.stripBase[l];
    orbx_keypoint_t *d_kps = v.kps; uint8_t *d_desc = v.desc; int32_t *d_counts = v.counts;
    if (prof) ORBX_HIP(hipEventRecord(ev[0], st));
    if (!skipPyr) {   // K1 (skipped when the pyramid was built ahead: then its level-wide blur was, too)
        launch_pyramid(h, v.imgs, v.pyr, B, stride, img_stride, st, v.lv0);
        unsigned m = 0;
        rc = launch_blur(h, h->d_pyr, &h->d_blur, &h->blurBytes, v.b0, B, st, &m);
        if (rc) return rc;
        h->blurMaskLast = m;
    }
    if (evPyrDone) ORBX_HIP(hipEventRecord(evPyrDone, st));
    if (p.orderKernel) hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, st);
    if (profFast) ORBX_HIP(hipEventRecord(ev[1], st));
    if (p.fastDoneAt == ORBX_FASTDONE_WITH_FAST) ORBX_HIP(hipEventRecord(h->evFastDone, st));
    OctSrc osrc = {};
    if (p.fused) {   // k_octree_pyr reads the FAST stage's cell lists in place
        osrc.cellCnt = v.cellCnt; osrc.cellRaw = v.cellRaw; osrc.slots = v.slots; osrc.slotsPerImg = h->sp.slotsPerImg;
        osrc.totalCells = h->sp.totalCells; osrc.iniTh = h->ini_th; osrc.minTh = h->min_th; osrc.candCntOut = v.candCnt;
        osrc.sparseFlag = v.sparse; osrc.sparsePerCell = p.sparsePerCell; osrc.candOut = v.cand;
        osrc.sparseSeen = p.sparseHint == ORBX_HINT_OCT_SRC ? h->d_sparseSeen : nullptr; osrc.callSeq = h->callSeq;
        h->candStale = std::max(h->candStale, v.b0 + B);
    }
    FastHist fhist = {};
    if (p.histOct) {   // the FAST stage histograms its emissions for the quad-tree
        fhist.cnt = h->d_histCnt; fhist.best = h->d_histBest; fhist.stride = h->sp.histStride; fhist.tab = h->d_tab;
        osrc.histCnt = h->d_histCnt; osrc.histBest = h->d_histBest; osrc.histStride = h->sp.histStride;
    }
    int pow2 = 1;
    while (pow2 < h->sp.maxNodeCap) pow2 <<= 1;
    int maxCellsL = 0;
    for (int l = 0; l < nl; l++) maxCellsL = std::max(maxCellsL, h->sp.geom[l].ncells);
    const int scratch = std::max(4 * h->sp.maxNodeCap, maxCellsL + 1);
    const size_t ldsOct = std::max(h->sp.octPyrLdsBytes, h->sp.octLdsBytes);
    hipStream_t s2 = h->side[1];   // the second stream of the early quad-tree and of the split call
    {   // K2
        const int32_t *spf = p.rowFlags ? v.sparse : (const int32_t *)nullptr;
        const int sA = p.earlyLv ? h->sp.stripBase[p.earlyLv] : 0;
        if (p.earlyLv) {   // the strips of the levels [0, earlyLv) first; their quad-tree starts beside the FAST of the rest
            hipLaunchKernelGGL(k_fast_strips, dim3((sA + FAST_WAVES - 1) / FAST_WAVES, B), dim3(64 * FAST_WAVES), 0, st,
                               v.pyr, h->sp.pyrImgBytes, h->d_geom, nl, sA, h->sp.totalCells, v.cellCnt, v.cellRaw,
                               v.slots, h->sp.slotsPerImg, h->ini_th, h->min_th, sb, spf, 0, p.compact ? 1 : 0, v.lv0);
            ORBX_HIP(hipEventRecord(h->evGather, st));
            ORBX_HIP(hipStreamWaitEvent(s2, h->evGather, 0));
            ORBX_OCT_PYR_ON(s2, dim3(B, p.earlyLv), 0, 0, 0, osrc);
            ORBX_HIP(hipEventRecord(h->evOctA, s2));
        }
        if (p.strips && h->sp.totalStrips > sA)
            hipLaunchKernelGGL(k_fast_strips, dim3((h->sp.totalStrips - sA + FAST_WAVES - 1) / FAST_WAVES, B), dim3(64 * FAST_WAVES), 0, st,
                               v.pyr, h->sp.pyrImgBytes, h->d_geom, nl, h->sp.totalStrips, h->sp.totalCells, v.cellCnt, v.cellRaw,
                               v.slots, h->sp.slotsPerImg, h->ini_th, h->min_th, sb, spf, sA, p.compact ? 1 : 0, v.lv0);
        if (p.compact && p.sparseForm == 1) {   // the flagged (image, level)s: the strip kernel's compaction twin
            hipLaunchKernelGGL(k_fast_strips_sparse, dim3((h->sp.totalStrips + FAST_WAVES - 1) / FAST_WAVES, B), dim3(64 * FAST_WAVES), 0, st,
                               v.pyr, h->sp.pyrImgBytes, h->d_geom, nl, h->sp.totalStrips, h->sp.totalCells, v.cellCnt, v.cellRaw,
                               v.slots, h->sp.slotsPerImg, h->ini_th, h->min_th, sb, v.sparse, v.lv0);
        } else if (p.compact) {   // ORBX_OPT_SPARSE_FORM = 2: the cell kernel's compaction form (+ the queue of 16-bit entries behind a wave's tiles)
            const int ldsw = h->sp.fastLdsPerWave + ((32 * h->sp.fastTileRows + 15) & ~15);
            ORBX_LAUNCH_FAST_ES(true, ldsw);
        }
        if (p.fastCells) ORBX_LAUNCH_FAST_ES(false, h->sp.fastLdsPerWave);
    }
    if (profFast) ORBX_HIP(hipEventRecord(ev[2], st));
    if (p.fastDoneAt == ORBX_FASTDONE_BEHIND_FAST) ORBX_HIP(hipEventRecord(h->evFastDone, st));
    {   // K3
        if (p.gather)
            hipLaunchKernelGGL(k_gather, dim3((h->sp.totalCells + GATHER_CELLS_PER_BLOCK - 1) / GATHER_CELLS_PER_BLOCK, B),
                               dim3(256), 0, st, h->d_geom, nl, h->sp.totalCells, v.cellCnt, v.cellRaw, v.slots,
                               h->sp.slotsPerImg, v.cand, h->sp.keysPerImg, v.candCnt, h->ini_th, h->min_th, cb, v.sparse, p.sparsePerCell,
                               p.sparseHint == ORBX_HINT_GATHER ? h->d_sparseSeen : (int32_t *)nullptr, h->callSeq);
        if (p.aSplit > 0) {   // scratch records of the levels [a, nl)
            const size_t need = (size_t)h->pB * cap * 60;
            if (h->splitBytes < need) {
                ORBX_HIP(hipStreamSynchronize(st));
                ORBX_HIP(hipStreamSynchronize(s2));
                hipFree(h->d_kpsB); hipFree(h->d_descB); h->d_kpsB = nullptr; h->d_descB = nullptr; h->splitBytes = 0;
                ORBX_HIP(scratch_malloc(&h->d_kpsB, (size_t)h->pB * cap * sizeof(orbx_keypoint_t)));
                ORBX_HIP(scratch_malloc(&h->d_descB, (size_t)h->pB * cap * 32));
                h->splitBytes = need;
            }
        }
        // (k_octree_pyr: a level whose tree outgrows the count pyramid is redone by the same block with the exact form: one launch)
        switch (p.octForm) {
        case ORBX_OCT_EXACT:
            ORBX_OCT_LAUNCH_ON(st, k_octree, k_octree_wide, dim3(B, nl), h->sp.octLdsBytes, h->d_geom, nl, v.cand, v.nodeOf,
                               h->sp.keysPerImg, v.candCnt, v.lvlKp, h->sp.lvlKpCap, v.lvlCnt, h->d_tab, h->sp.maxNodeCap, pow2,
                               scratch, p.octPhase);
            break;
        case ORBX_OCT_BIG: {
            OctBig big = {};
            // the kernels index this scratch by the chunk-local image: chunks that run side by side on two streams get disjoint slots
            big.part = h->d_octPart + v.octSlot0 * OCT_BIG_K * (size_t)h->sp.octDeepMax; big.leaf = h->d_octLeaf + v.octSlot0 * (size_t)h->sp.octPyrWords;
            big.best = h->d_octBest + v.octSlot0 * (size_t)h->sp.maxNodeCap; big.state = h->d_octState + v.octSlot0 * 4;
            big.K = OCT_BIG_K; big.deepMax = h->sp.octDeepMax; big.pyrMax = h->sp.octPyrWords;
            for (int l = 0; l < nl; l++) if (((unsigned)p.bigMask >> l) & 1u) big.levelOf[big.nBig++] = l;
            // large levels: K workgroups histogram, the last one to arrive runs the passes; the same launch carries the other
            // levels (one workgroup each, listed behind the large ones) ...
            int nall = big.nBig;
            for (int l = 0; l < nl; l++) if (!(((unsigned)p.bigMask >> l) & 1u)) big.levelOf[nall++] = l;
            ORBX_OCT_LAUNCH_ON(st, k_octree_big<1>, k_octree_big_wide<1>, dim3(OCT_BIG_K, nl, B), ldsOct, h->d_geom, nl, v.cand, h->sp.keysPerImg,
                               v.candCnt, v.lvlKp, h->sp.lvlKpCap, v.lvlCnt, h->d_tab, h->sp.maxNodeCap, pow2, h->sp.octPyrWords,
                               v.octFallback, v.nodeOf, scratch, big);
            // ... then K workgroups elect the best key per node, the last one writes the level's keypoints
            ORBX_OCT_LAUNCH_ON(st, k_octree_big<2>, k_octree_big_wide<2>, dim3(OCT_BIG_K, big.nBig, B), ldsOct, h->d_geom, nl, v.cand, h->sp.keysPerImg,
                               v.candCnt, v.lvlKp, h->sp.lvlKpCap, v.lvlCnt, h->d_tab, h->sp.maxNodeCap, pow2, h->sp.octPyrWords,
                               v.octFallback, v.nodeOf, scratch, big);
            break;
        }
        case ORBX_OCT_EARLY:   // the quad-tree of the levels [0, earlyLv) is already running on the second stream (started behind their strips)
            ORBX_OCT_PYR_ON(st, dim3(B, nl - p.earlyLv), 0, 0, p.earlyLv, osrc);
            ORBX_HIP(hipStreamWaitEvent(st, h->evOctA, 0));
            break;
        case ORBX_OCT_SPLIT:
            // Split call: the quad-tree of the large levels [0, a) - one workgroup per level walking a serial chain, the critical
            // path of this stage - moves to a second stream, and the small levels [a, nl) go ahead on the caller's stream:
            // their quad-tree, then their descriptors (a VALU-bound kernel that fills the GPU) into scratch arrays, beside that
            // chain.  The descriptors of [0, a) follow when both are done and move the scratch records behind their own.
            ORBX_HIP(hipEventRecord(h->evGather, st));
            ORBX_HIP(hipStreamWaitEvent(s2, h->evGather, 0));
            ORBX_OCT_PYR_ON(s2, dim3(B, p.aSplit), 0, 0, 0, osrc);
            ORBX_HIP(hipEventRecord(h->evOctA, s2));
            ORBX_OCT_PYR_ON(st, dim3(B, nl - p.aSplit), 0, 0, p.aSplit, osrc);
            break;
        default: {   // ORBX_OCT_SINGLE: one workgroup per level, one launch - or, with a shared sweep, several for a large level
            OctSrc os = osrc;
            if (p.sweepSlices) {
                for (int l = 0; l < nl; l++) os.nslice[l] = (unsigned char)p.nslice[l];
                os.partCnt = h->d_octPartCnt + v.octSlot0 * OCT_MAX_SLICES * (size_t)h->sp.octSliceStride;
                os.partBest = h->d_octPartBest + v.octSlot0 * OCT_MAX_SLICES * (size_t)h->sp.octSliceStride;
                os.sliceState = h->d_octSliceState + v.octSlot0;
                os.maxSlices = OCT_MAX_SLICES; os.partStride = h->sp.octSliceStride;
            }
            dim3 ogrid(B, nl);
            if (p.sweepShared) {   // linear grid: every slice of the large levels in front of the small levels
                os.linear = 1; os.nImages = B;
                int tot = 0;
                for (int l = 0; l <= ORBX_MAX_LEVELS; l++) { os.blkPrefix[l] = tot; if (l < nl) tot += B * std::max(1, (int)os.nslice[l]); }
                ogrid = dim3(tot);
            }
            ORBX_OCT_PYR_ON(st, ogrid, p.octStop, p.octPhase, 0, os);
        }
        }
    }
    if (prof) ORBX_HIP(hipEventRecord(ev[3], st));
    if (p.fastDoneAt == ORBX_FASTDONE_BEHIND_OCT) ORBX_HIP(hipEventRecord(h->evFastDone, st));
    {   // K4 (one instance per flavour of the Gaussian's column rounding: the default pays nothing for the other)
        const bool sse2 = h->flavour.gauss_rounding == ORBX_GAUSS_ROUND_SSE2;
        // ORBX_OPT_DESC_LDS_PAD (KB): unused dynamic LDS per workgroup = fewer resident k_describe workgroups per CU, i.e. wave slots
        // left for the pyramid kernels that run beside it in a pipelined step (tuning only)
        const size_t descPad = (size_t)p.descLdsPad;
        const bool ftaps = h->flavour.gauss_rounding == ORBX_GAUSS_FIXED_TAPS;
        const uint32_t taps = gauss_taps_packed(h);
        const auto kDesc = p.aSplit > 0 ? (ftaps ? k_describe<ORBX_GAUSS_FIXED_TAPS, true> : sse2 ? k_describe<ORBX_GAUSS_ROUND_SSE2, true> : k_describe<ORBX_GAUSS_ROUND_HALF_UP, true>)
                                        : (ftaps ? k_describe<ORBX_GAUSS_FIXED_TAPS, false> : sse2 ? k_describe<ORBX_GAUSS_ROUND_SSE2, false> : k_describe<ORBX_GAUSS_ROUND_HALF_UP, false>);
        const uint8_t *blurp = h->blurMaskLast ? h->d_blur + (size_t)v.b0 * h->sp.pyrImgBytes : nullptr;
        // a describing block belongs to one level: blocks for the most keypoints every level can return (desc_level_blocks)
        const auto bound = [&](int l) { return std::max(h->sp.geom[l].N + 2, 4 * h->sp.geom[l].nIni); };
        if (p.aSplit > 0) {
            int boundB = 0;
            for (int l = p.aSplit; l < nl; l++) boundB += bound(l);
            const int maxoB = std::min(cap, boundB);
            orbx_keypoint_t *kB = h->d_kpsB + (size_t)v.b0 * cap;
            uint8_t *dB = h->d_descB + (size_t)v.b0 * cap * 32;
            DescGroup gB = {p.aSplit, nl, 0, 0, nullptr, nullptr};
            const int nbB = gB.copyBlock0 = desc_level_blocks(p.aSplit, nl, bound, gB.blk0);
            gB.taps = taps;
            hipLaunchKernelGGL(kDesc, dim3(nbB, B), dim3(64 * DESC_WAVES), descPad, st, v.pyr, h->sp.pyrImgBytes, h->d_geom, nl,
                               v.lvlKp, h->sp.lvlKpCap, v.lvlCnt, kB, dB, d_counts, cap, (uint8_t *)nullptr, blurp, h->blurMaskLast, gB, v.lv0);
            ORBX_HIP(hipStreamWaitEvent(st, h->evOctA, 0));
            DescGroup gA = {0, p.aSplit, 1, 0, kB, dB};
            const int nbA = gA.copyBlock0 = desc_level_blocks(0, p.aSplit, bound, gA.blk0);
            gA.taps = taps;
            hipLaunchKernelGGL(kDesc, dim3(nbA + (maxoB + DESC_COPY_PER_BLOCK - 1) / DESC_COPY_PER_BLOCK, B), dim3(64 * DESC_WAVES), descPad, st,
                               v.pyr, h->sp.pyrImgBytes, h->d_geom, nl, v.lvlKp, h->sp.lvlKpCap, v.lvlCnt, d_kps, d_desc, d_counts, cap,
                               (uint8_t *)nullptr, blurp, h->blurMaskLast, gA, v.lv0);
        } else {
            DescGroup gAll = {0, nl, 1, 0, nullptr, nullptr};
            const int nb = gAll.copyBlock0 = desc_level_blocks(0, nl, bound, gAll.blk0);
            gAll.taps = taps;
            gAll.hostDelta = h->descHostDelta;   // latency form: records also stored into their pinned host twin
            hipLaunchKernelGGL(kDesc, dim3(nb, B), dim3(64 * DESC_WAVES), descPad, st, v.pyr, h->sp.pyrImgBytes, h->d_geom, nl,
                               v.lvlKp, h->sp.lvlKpCap, v.lvlCnt, d_kps, d_desc, d_counts, cap, h->d_dbgBlur, blurp, h->blurMaskLast, gAll, v.lv0);
        }
    }
    if (prof) ORBX_HIP(hipEventRecord(ev[4], st));
    if (p.fastDoneAt == ORBX_FASTDONE_BEHIND_DESC) ORBX_HIP(hipEventRecord(h->evFastDone, st));
    return ORBX_OK;
}
#undef ORBX_LAUNCH_FAST_ES
#undef ORBX_LAUNCH_FAST
#undef ORBX_OCT_PYR_ON
#undef ORBX_OCT_LAUNCH_ON

// A batch runs as up to ORBX_MAX_CHUNKS chunks of images.  Chunk 0 goes to the caller's stream, the others to the handle's side
// streams, and chunk c's pyramid waits for chunk c-1's: the memory-bound pyramid and the latency-bound gather / quad-tree of one
// chunk then overlap the issue-bound FAST and descriptor kernels of another (the kernels are the same, per-image results do not
// depend on the chunking), and the caller's stream waits for the side streams at the end, so the call keeps its stream semantics.
static int launch_pipeline(orbx_extractor *h, const uint8_t *d_imgs, int B, int w, int hgt, int stride,
                           size_t img_stride, orbx_keypoint_t *d_kps, uint8_t *d_desc, int32_t *d_counts,
                           int cap, hipStream_t st, bool skipPyr = false, Level0 lv0 = Level0{}) {
    // where level 0 of this call's pyramid lives: a pyramid built ahead brought its own answer with its buffer (the caller rotated it
    // in), any other call overwrites d_pyr and says it here (lv0.base != NULL: in-place input; every other entry point copies)
    if (!skipPyr) h->lv0 = lv0;
    h->lv0Stale = h->lv0.base ? B : 0;
    // profiling 1: events at every stage boundary; 2: only around the FAST stage (an event costs ~4.5 us of idle GPU, so
    // a throughput measurement brackets just the kernel it reports); mode 3 = mode 2 on every 4th call only
    const bool prof = h->profiling == 1, profFast = h->profiling != 0 && (h->profiling != 3 || (h->prof_calls++ & 3) == 0);
    (void)hipGetLastError();  // drop stale errors of other HIP users in this process
    hipEvent_t *ev = nullptr;
    if (profFast) {
        const int slot = h->ev_head % ORBX_EV_RING;
        if (h->ev_pending[slot]) { int rc = harvest_events(h, slot); if (rc) return rc; }
        ev = h->ev[slot];
    }
    // developer knob 8: n >= 2 = n chunks (default: one - measured on 64 stereo frames, two chunks: 773 us against 742, the
    // latency-bound gather / quad-tree do not shrink with the chunk and the pyramid slows the FAST it overlaps by as much as it gains).
    const int nch = chunk_count(h->opt, B, prof, skipPyr);
    h->lastChunks = nch;
    h->candStale = 0;
    h->callSeq = (int)((unsigned)h->callSeq + 1u);   // wraps (compared by unsigned distance)
    h->prevPyrValid = skipPyr ? 1 : 0;   // d_pyr is overwritten unless this call took a pyramid built ahead (then d_pyrAlt keeps the previous one)
    h->framesStale = (!pyramid_fused_all(h) && h->nlevels > 1) ? B : 0;   // frames of levels >= 1: written on demand (ensure_frames)
    int b0 = 0;
    for (int c = 0; c < nch; c++) {
        const int Bc = (B - b0) / (nch - c);
        const ChunkView v = chunk_view(h, d_imgs, img_stride, d_kps, d_desc, d_counts, cap, b0);
        hipStream_t sc = c == 0 ? st : h->side[(c - 1) % ORBX_SIDE_STREAMS];
        if (c > 0) ORBX_HIP(hipStreamWaitEvent(sc, h->evPyr[c - 1], 0));
        int rc = launch_chunk(h, v, Bc, stride, img_stride, cap, sc, ev, prof && c == 0, profFast && c == 0, c + 1 < nch ? h->evPyr[c] : nullptr, skipPyr);
        if (rc) return rc;
        b0 += Bc;
    }
    for (int s = 0; s < std::min(nch - 1, ORBX_SIDE_STREAMS); s++) {   // the caller's stream carries on when every side stream is done
        ORBX_HIP(hipEventRecord(h->evJoin[s], h->side[s]));
        ORBX_HIP(hipStreamWaitEvent(st, h->evJoin[s], 0));
    }
    if (profFast) { h->ev_pending[h->ev_head % ORBX_EV_RING] = (unsigned char)(h->profiling == 3 ? 2 : h->profiling); h->ev_head++; }
    ORBX_HIP(hipGetLastError());
    h->last_stream = st;
    h->last_valid = 1;
    h->lastB = B;
    (void)w; (void)hgt;
    return ORBX_OK;
}

// In-place input: d_imgs is the base of B images in the layout of orbx_level0_layout (the padded level 0 of the plan; margins the
// caller's, contents unspecified).  Checked against the plan, then restated as the dense call the copy path would get - pixel (0,0) of
// image 0, rows pstride apart - plus *lv0, set iff the call may read level 0 where it is (level0_in_place_ok).
static int padded_input(const orbx_extractor *h, const char *fn, const uint8_t **d_imgs, int B, int nch, int *stride, size_t image_stride_bytes, Level0 *lv0) {
    const LevelGeom &g0 = h->sp.geom[0];
    const size_t need = level0_image_bytes(g0);
    if (image_stride_bytes < need || (image_stride_bytes & 63) || ((uintptr_t)*d_imgs & 63)) {
        orbx_set_error("%s: images of the orbx_level0_layout are %zu bytes, 64-byte aligned and a multiple of 64 bytes apart (got %zu bytes apart)", fn, need,
                       image_stride_bytes);
        return ORBX_ERR_ARG;
    }
    *lv0 = level0_in_place_ok(h, B, nch) ?Level0{*d_imgs, image_stride_bytes} : Level0{};
    *d_imgs += (size_t)ORBX_EDGE * g0.pstride + ORBX_EDGE;
    *stride = g0.pstride;
    return ORBX_OK;
}

static int extract_batch_device_impl(orbx_extractor_t *h, const char *fn, bool padded, const uint8_t *d_imgs, int B, int w, int hgt,
                                     int stride, size_t image_stride_bytes, orbx_keypoint_t *d_kps,
                                     uint8_t *d_desc, int32_t *d_counts, int cap, void *stream) {
    if (!h || !d_imgs || !d_kps || !d_desc || !d_counts || B < 1 || w < 1 || hgt < 1 || (!padded && stride < w) || cap < 1) {
        orbx_set_error("%s: bad arguments", fn);
        return ORBX_ERR_ARG;
    }
    ORBX_HIP(hipSetDevice(h->device));
    int rc = ensure_plan(h, w, hgt, B);
    if (rc) return rc;
    Level0 lv0 = {};
    // (decided for the call that builds its own pyramid, in launch_pipeline's chunks: one that takes a pyramid built ahead keeps what
    // the prefetch decided for that buffer and ignores this)
    if (padded) { rc = padded_input(h, fn, &d_imgs, B, chunk_count(h->opt, B, h->profiling == 1, false), &stride, image_stride_bytes, &lv0); if (rc) return rc; }
    hipStream_t st = (hipStream_t)stream;  // NULL = the HIP default (null) stream, as in every HIP API
    // the pyramid of exactly this batch was built ahead (orbx_extract_batch_device_prefetch): take that buffer, skip K1
    const bool three = h->pyrBuffers == 3;
    const bool ahead = h->pfValid && (three ? h->d_pyrNext != nullptr : h->d_pyrAlt != nullptr) && h->pfImgs == d_imgs && h->pfB == B && h->pfW == w && h->pfH == hgt && h->pfStride == stride &&
                       h->pfImgStride == image_stride_bytes && (h->pfPadded != 0) == padded && h->opt[9] == 0;
    h->pfValid = 0;
    h->prevPyrValid = ahead ? 1 : 0;   // the buffers swap: the other one keeps the previous call's pyramid until the next one is built into it
    if (ahead) {   // (where level 0 of a pyramid lives - Level0 - moves with its buffer)
        if (three) {   // previous <- current <- next <- (old previous: its matcher was issued on the side stream before the next prefetch is)
            if (h->pyrAltBytes < h->sp.pyrImgBytes * (size_t)h->pB) {   // first rotation: the "previous" buffer does not exist yet
                ORBX_HIP(hipStreamSynchronize(h->side[0]));
                hipFree(h->d_pyrAlt); h->d_pyrAlt = nullptr;
                ORBX_HIP(scratch_malloc(&h->d_pyrAlt, h->sp.pyrImgBytes * (size_t)h->pB));
                h->pyrAltBytes = h->sp.pyrImgBytes * (size_t)h->pB;
            }
            uint8_t *oldPrev = h->d_pyrAlt;
            h->d_pyrAlt = h->d_pyr; h->d_pyr = h->d_pyrNext; h->d_pyrNext = oldPrev;
            h->lv0Alt = h->lv0; h->lv0 = h->lv0Next; h->lv0Next = Level0{};
        } else {
            std::swap(h->d_pyr, h->d_pyrAlt);
            std::swap(h->lv0, h->lv0Alt);
        }
        std::swap(h->d_blur, h->d_blurAlt); std::swap(h->blurBytes, h->blurAltBytes); std::swap(h->blurMaskLast, h->blurMaskAlt);
        ORBX_HIP(hipStreamWaitEvent(st, h->evPrefetch, 0));
    }
    return launch_pipeline(h, d_imgs, B, w, hgt, stride, image_stride_bytes, d_kps, d_desc, d_counts, cap, st, ahead, lv0);
}
extern "C" int orbx_extract_batch_device(orbx_extractor_t *h, const uint8_t *d_imgs, int B, int w, int hgt,
                                         int stride, size_t image_stride_bytes, orbx_keypoint_t *d_kps,
                                         uint8_t *d_desc, int32_t *d_counts, int cap, void *stream) {
    return extract_batch_device_impl(h, "orbx_extract_batch_device", false, d_imgs, B, w, hgt, stride, image_stride_bytes, d_kps, d_desc, d_counts, cap, stream);
}
extern "C" int orbx_extract_batch_device_padded(orbx_extractor_t *h, const uint8_t *d_level0, int B, int w, int hgt, size_t image_stride_bytes,
                                                orbx_keypoint_t *d_kps, uint8_t *d_desc, int32_t *d_counts, int cap, void *stream) {
    return extract_batch_device_impl(h, "orbx_extract_batch_device_padded", true, d_level0, B, w, hgt, 0, image_stride_bytes, d_kps, d_desc, d_counts, cap, stream);
}

// Software pipelining across batches: start ComputePyramid of the NEXT batch now, into the handle's second pyramid buffer, on a
// stream of the handle's own.  It is ordered behind the FAST stage of the extraction call issued last, i.e. it runs beside that
// call's gather / quad-tree (latency-bound), descriptors and the stereo matcher instead of in front of the next call's FAST.
static int prefetch_impl(orbx_extractor_t *h, const char *fn, bool padded, const uint8_t *d_imgs, int B, int w, int hgt, int stride,
                         size_t image_stride_bytes, void *side_stream) {
    if (!h || !d_imgs || B < 1 || w < 1 || hgt < 1 || (!padded && stride < w)) { orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    int rc = ensure_plan(h, w, hgt, B);
    if (rc) return rc;
    Level0 lv0 = {};
    if (padded) { rc = padded_input(h, fn, &d_imgs, B, 1, &stride, image_stride_bytes, &lv0); if (rc) return rc; }   // one pyramid launch of the whole batch
    const size_t need = h->sp.pyrImgBytes * (size_t)h->pB;
    const bool three = h->pyrBuffers == 3;
    uint8_t **tgt = three ? &h->d_pyrNext : &h->d_pyrAlt;
    size_t *tgtBytes = three ? &h->pyrNextBytes : &h->pyrAltBytes;
    if (*tgtBytes < need) {
        ORBX_HIP(hipStreamSynchronize(h->side[0]));
        hipFree(*tgt); *tgt = nullptr; *tgtBytes = 0;
        ORBX_HIP(scratch_malloc(tgt, need));
        *tgtBytes = need;
    }
    hipStream_t sd = side_stream ? (hipStream_t)side_stream : h->side[0];   // the caller's side stream (work it queued there comes first) or the handle's own
    if (!three) h->prevPyrValid = 0;   // two buffers: the pyramid built ahead overwrites the previous one (three: it has a buffer of its own)
    (void)hipGetLastError();
    if (h->pfUsed && h->last_valid) ORBX_HIP(hipStreamWaitEvent(sd, h->evFastDone, 0));   // (the first time there is no such event yet: the
    else if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));             //  second buffer is new, wait for the handle to be idle)
    h->pfUsed = 1;
    launch_pyramid(h, d_imgs, *tgt, B, stride, image_stride_bytes, sd, lv0);
    (three ? h->lv0Next : h->lv0Alt) = lv0;
    rc = launch_blur(h, *tgt, &h->d_blurAlt, &h->blurAltBytes, 0, B, sd, &h->blurMaskAlt);
    if (rc) return rc;
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipEventRecord(h->evPrefetch, sd));
    h->pfValid = 1; h->pfImgs = d_imgs; h->pfB = B; h->pfW = w; h->pfH = hgt; h->pfStride = stride; h->pfImgStride = image_stride_bytes;
    h->pfPadded = padded;
    return ORBX_OK;
}
extern "C" int orbx_extract_batch_device_prefetch(orbx_extractor_t *h, const uint8_t *d_imgs, int B, int w, int hgt, int stride,
                                                  size_t image_stride_bytes, void *side_stream) {
    return prefetch_impl(h, "orbx_extract_batch_device_prefetch", false, d_imgs, B, w, hgt, stride, image_stride_bytes, side_stream);
}
extern "C" int orbx_extract_batch_device_padded_prefetch(orbx_extractor_t *h, const uint8_t *d_level0, int B, int w, int hgt,
                                                         size_t image_stride_bytes, void *side_stream) {
    return prefetch_impl(h, "orbx_extract_batch_device_padded_prefetch", true, d_level0, B, w, hgt, 0, image_stride_bytes, side_stream);
}

// Two (default) or three pyramid buffers.  With three, orbx_extract_batch_device_prefetch builds the next pyramid into a buffer of its
// own and the previous call's pyramid stays valid, so a pipeline may issue the pyramid of batch i+1 BEFORE the matcher of batch i-1 on
// its side stream (pipeline.FrontEnd(stereo_late=True): the matcher then runs beside the descriptor kernel instead of beside the
// quad-tree).  The buffer the next prefetch overwrites is the one the matcher issued before it (same stream) has read.
extern "C" int orbx_set_pyramid_buffers(orbx_extractor_t *h, int n) {
    if (!h || (n != 2 && n != 3)) { orbx_set_error("orbx_set_pyramid_buffers: 2 or 3"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
    for (int i = 0; i < ORBX_SIDE_STREAMS; i++) ORBX_HIP(hipStreamSynchronize(h->side[i]));
    h->pyrBuffers = n;
    h->pfValid = 0; h->prevPyrValid = 0;
    return ORBX_OK;
}

// Orders `stream` behind the FAST stage of the extraction call issued last on h (the event the pyramid built ahead waits for):
// what a caller queues on `stream` afterwards runs beside that call's gather / quad-tree / descriptor kernels, not beside its FAST.
extern "C" int orbx_stream_wait_fast_stage(orbx_extractor_t *h, void *stream) {
    if (!h) { orbx_set_error("orbx_stream_wait_fast_stage: bad arguments"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    if (h->pfUsed && h->last_valid) ORBX_HIP(hipStreamWaitEvent((hipStream_t)stream, h->evFastDone, 0));
    else if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));   // no event yet (nothing was built ahead so far): wait on the host
    return ORBX_OK;
}

// The handle's own side stream (the one pyramids are built ahead on when the caller names none).  A process has few hardware
// queues and the runtime deals streams to them round-robin: a stream the caller creates may share its queue with the caller's main
// stream and then overlaps nothing; this one was created next to the handle and is known to sit on a queue of its own.
extern "C" void *orbx_side_stream(orbx_extractor_t *h) { return h ? (void *)h->side[0] : nullptr; }

// ~2 ms of nothing on one wave: the "busy" side of the queue probe below (constant 100 MHz counter)
__global__ void k_spin(long long ticks) {
    const long long t0 = wall_clock64();
    for (int i = 0; i < 100000 && wall_clock64() - t0 < ticks; i++) __builtin_amdgcn_s_sleep(32);   // bounded whatever the counter does
}
// true iff a command on `cand` starts while `busy` is still occupied, i.e. the two streams do not share a hardware queue
static bool streams_independent(hipStream_t busy, hipStream_t cand, hipEvent_t eb, hipEvent_t ec) {
    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, busy, 200000ll);
    if (hipEventRecord(eb, busy) != hipSuccess) return false;
    hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, cand);
    if (hipEventRecord(ec, cand) != hipSuccess) return false;
    if (hipEventSynchronize(ec) != hipSuccess) return false;
    const bool indep = hipEventQuery(eb) == hipErrorNotReady;   // the spin is still running: the candidate did not wait behind it
    (void)hipEventSynchronize(eb);
    (void)hipGetLastError();
    return indep;
}
// The side stream of the handle, made sure NOT to share a hardware queue with `main_stream` (the stream the caller issues its
// extraction calls on).  The runtime deals streams to a handful of hardware queues round-robin and has no API that tells which;
// two streams on one queue run strictly in order, and the software pipeline (matcher of the previous batch, pyramid of the next on
// the side stream beside the caller's kernels) then overlaps nothing - seen on every handle after the first of a process (the second
// FrontEnd of bench.py: 1.53 instead of 1.13 ms per end-to-end step).  So the side stream is probed: a 2-ms one-wave spin goes to
// main_stream, an empty kernel to the candidate; the candidate is kept if its kernel ran while the spin was still going.  One-off,
// a few ms; the caller's stream is occupied for that long.  Returns the (possibly replaced) side stream.
extern "C" void *orbx_side_stream_for(orbx_extractor_t *h, void *main_stream) {
    if (!h) return nullptr;
    if (hipSetDevice(h->device) != hipSuccess) return (void *)h->side[0];
    hipStream_t ms = (hipStream_t)main_stream;
    hipEvent_t eb = nullptr, ec = nullptr;
    if (hipEventCreateWithFlags(&eb, hipEventDisableTiming) != hipSuccess || hipEventCreateWithFlags(&ec, hipEventDisableTiming) != hipSuccess) {
        if (eb) hipEventDestroy(eb);
        return (void *)h->side[0];
    }
    (void)hipStreamSynchronize(ms);
    (void)hipStreamSynchronize(h->side[0]);
    if (!streams_independent(ms, h->side[0], eb, ec)) {
        std::vector<hipStream_t> tried;
        hipStream_t found = nullptr;
        for (int i = 0; i < 12 && !found; i++) {
            hipStream_t c = nullptr;
            if (hipStreamCreateWithFlags(&c, hipStreamNonBlocking) != hipSuccess) break;
            if (streams_independent(ms, c, eb, ec) && streams_independent(c, h->side[1], eb, ec)) found = c;
            else tried.push_back(c);
        }
        for (hipStream_t c : tried) hipStreamDestroy(c);
        if (found) {
            if (h->st_stream == h->side[0]) h->st_stream = nullptr;       // (nothing may keep the handle of the stream that goes away)
            if (h->last_valid && h->last_stream == h->side[0]) h->last_valid = 0;
            hipStreamDestroy(h->side[0]);
            h->side[0] = found;
            h->pfValid = 0; h->prevPyrValid = 0;
        }
    }
    hipEventDestroy(eb); hipEventDestroy(ec);
    (void)hipGetLastError();
    return (void *)h->side[0];
}
#ifdef ORBX_DEVELOPER
// include/orbx_dev.h: hold `stream` back by one k_spin (tests/test_stream_order_gpu.py).  Launches nothing else and waits for nothing.
extern "C" int orbx_debug_stall_stream(void *stream, int microseconds, int device) {
    if (microseconds < 1 || microseconds > 50000 || device < 0) { orbx_set_error("orbx_debug_stall_stream: 1 .. 50000 microseconds"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(device));
    hipLaunchKernelGGL(k_spin, dim3(1), dim3(64), 0, (hipStream_t)stream, 100ll * microseconds);   // 100 ticks of the wall clock per microsecond
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}
// include/orbx_dev.h: the streams a call on h (and a matcher call of this thread) issues work on, read only, no HIP call
extern "C" int orbx_debug_streams(orbx_extractor_t *h, void **out, int n_out) {
    if (!out || n_out != 5) { orbx_set_error("orbx_debug_streams: bad arguments"); return ORBX_ERR_ARG; }
    out[0] = h ? (void *)h->stream : nullptr;
    out[1] = h ? (void *)h->side[0] : nullptr;
    out[2] = h ? (void *)h->side[1] : nullptr;
    out[3] = orbx_internal_arena_stream();
    out[4] = orbx_internal_match_scratch_stream();
    return ORBX_OK;
}
#endif

static int ensure_staging(orbx_extractor *h, size_t in_bytes, int B, int cap) {
    if (h->d_in_bytes < in_bytes) {
        hipFree(h->d_in); h->d_in = nullptr; h->d_in_bytes = 0;
        ORBX_HIP(scratch_malloc(&h->d_in, in_bytes));
        h->d_in_bytes = in_bytes;
    }
    if (h->out_cap < cap || h->out_B < B) {
        hipFree(h->d_kps); hipFree(h->d_desc); hipFree(h->d_counts);
        h->d_kps = nullptr; h->d_desc = nullptr; h->d_counts = nullptr;
        const int nb = std::max(B, h->out_B), nc = std::max(cap, h->out_cap);
        ORBX_HIP(scratch_malloc(&h->d_kps, sizeof(orbx_keypoint_t) * (size_t)nb * nc));
        ORBX_HIP(scratch_malloc(&h->d_desc, (size_t)32 * nb * nc));
        ORBX_HIP(scratch_malloc(&h->d_counts, sizeof(int32_t) * nb));
        // pinned mirrors: the results of a host-API call come down in three copies and ONE synchronisation
        if (h->h_kps) { hipHostFree(h->h_kps); hipHostFree(h->h_desc); hipHostFree(h->h_counts); h->h_kps = nullptr; h->h_desc = nullptr; h->h_counts = nullptr; }
        ORBX_HIP(scratch_host_malloc((void **)&h->h_kps, sizeof(orbx_keypoint_t) * (size_t)nb * nc, hipHostMallocDefault));
        ORBX_HIP(scratch_host_malloc((void **)&h->h_desc, (size_t)32 * nb * nc, hipHostMallocDefault));
        ORBX_HIP(scratch_host_malloc((void **)&h->h_counts, sizeof(int32_t) * nb, hipHostMallocDefault));
        h->out_cap = nc; h->out_B = nb;
    }
    return ORBX_OK;
}

extern "C" int orbx_extract_batch(orbx_extractor_t *h, const uint8_t *const *imgs, int B, int w, int hgt,
                                  int stride, orbx_keypoint_t *kps, uint8_t *desc, int cap, int *n_out) {
    if (!h || !imgs || !kps || !desc || !n_out || B < 1 || cap < 1) {
        orbx_set_error("orbx_extract_batch: bad arguments");
        return ORBX_ERR_ARG;
    }
    if (w <= 0 || hgt <= 0) {  // empty image: silent return (:1046-1047)
        for (int b = 0; b < B; b++) n_out[b] = 0;
        return ORBX_OK;
    }
    if (stride < w) { orbx_set_error("stride < width"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    int rc = ensure_plan(h, w, hgt, B);
    if (rc) return rc;
    // One linear copy per image with the caller's row stride kept on the device (the kernels take a stride):
    // a 2-D copy of rows whose width is not a multiple of 4 bytes (1241!) runs ~100x slower than a linear one.
    const size_t span = (size_t)stride * (hgt - 1) + w;
    const size_t img_bytes = (span + 255) & ~(size_t)255;
    rc = ensure_staging(h, img_bytes * B, B, cap);
    if (rc) return rc;
    const int dcap = h->out_cap;
    for (int b = 0; b < B; b++) {
        if (!imgs[b]) { orbx_set_error("imgs[%d] is NULL", b); return ORBX_ERR_ARG; }
        ORBX_HIP(hipMemcpyAsync(h->d_in + img_bytes * b, imgs[b], span, hipMemcpyHostToDevice, h->stream));
    }
    rc = launch_pipeline(h, h->d_in, B, w, hgt, stride, img_bytes, h->d_kps, h->d_desc, h->d_counts, dcap, h->stream);
    if (rc) return rc;
    ORBX_HIP(hipMemcpyAsync(h->h_counts, h->d_counts, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(hipMemcpyAsync(h->h_kps, h->d_kps, sizeof(orbx_keypoint_t) * (size_t)B * dcap, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(hipMemcpyAsync(h->h_desc, h->d_desc, (size_t)32 * B * dcap, hipMemcpyDeviceToHost, h->stream));
    ORBX_HIP(hipStreamSynchronize(h->stream));
    int status = ORBX_OK;
    for (int b = 0; b < B; b++) {
        int n = h->h_counts[b];
        if (n > cap) { n = cap; status = ORBX_ERR_CAPACITY; orbx_set_error("frame %d produced %d keypoints, cap %d", b, h->h_counts[b], cap); }
        n_out[b] = n;
        if (n > 0) {
            memcpy(kps + (size_t)b * cap, h->h_kps + (size_t)b * dcap, sizeof(orbx_keypoint_t) * n);
            memcpy(desc + (size_t)b * cap * 32, h->h_desc + (size_t)b * dcap * 32, (size_t)32 * n);
        }
    }
    return status;
}

// One stereo frame host to host in ONE call: what the reference's stereo Frame constructor does with two extractor threads and a CPU
// matcher (src/Frame.cc:78-84: ExtractORB(0, imLeft) || ExtractORB(1, imRight), then ComputeStereoMatches, :481-655).  Both images
// go up, are extracted as one batch of two on this handle (slots 0 / 1), matched on the device, and everything comes down behind ONE
// synchronisation: no second extractor, no re-upload of the keypoints the extractor just produced.
// The body of orbx_stereo_frame: host images `left` / `right` are uploaded into the handle's staging first; d_pair != NULL: the pair
// is in HBM already (image 1 at d_pair + pair_img_bytes, work queued on the handle's stream before this call produces it).
static int stereo_frame_run(orbx_extractor *h, const uint8_t *left, const uint8_t *right, const uint8_t *d_pair, int w, int hgt,
                            int stride, size_t pair_img_bytes, float mbf, float mb, int cap, orbx_keypoint_t *kl, uint8_t *dl, int *nl,
                            orbx_keypoint_t *kr, uint8_t *dr, int *nr, float *uright, float *depth, int *nmatch) {
    ORBX_HIP(hipSetDevice(h->device));
    int rc = ensure_plan(h, w, hgt, 2);
    if (rc) return rc;
    const size_t span = (size_t)stride * (hgt - 1) + w, img_bytes = (span + 255) & ~(size_t)255;
    rc = ensure_staging(h, d_pair ? 0 : img_bytes * 2, 2, cap);
    if (rc) return rc;
    const int dcap = h->out_cap;
    if (h->sfr_cap < dcap) {
        hipFree(h->d_sfr); h->d_sfr = nullptr;
        if (h->h_sfr) { hipHostFree(h->h_sfr); h->h_sfr = nullptr; }
        h->sfr_cap = 0;
        ORBX_HIP(scratch_malloc(&h->d_sfr, sizeof(float) * (2 * (size_t)dcap + 4)));
        ORBX_HIP(scratch_host_malloc((void **)&h->h_sfr, sizeof(float) * (2 * (size_t)dcap + 4), hipHostMallocDefault));
        h->sfr_cap = dcap;
    }
    hipStream_t st = h->stream;
    if (!d_pair) {
        ORBX_HIP(hipMemcpyAsync(h->d_in, left, span, hipMemcpyHostToDevice, st));
        ORBX_HIP(hipMemcpyAsync(h->d_in + img_bytes, right, span, hipMemcpyHostToDevice, st));
    }
    rc = launch_pipeline(h, d_pair ? d_pair : h->d_in, 2, w, hgt, stride, d_pair ? pair_img_bytes : img_bytes, h->d_kps, h->d_desc,
                         h->d_counts, dcap, st);
    if (rc) return rc;
    float *d_ur = h->d_sfr, *d_dp = h->d_sfr + dcap;
    int32_t *d_nm = (int32_t *)(h->d_sfr + 2 * (size_t)dcap);
    rc = orbm_stereo_batch_device(h, h, 1, 0, 1, h->d_kps, h->d_desc, h->d_counts, h->d_kps + dcap, h->d_desc + (size_t)dcap * 32,
                                  h->d_counts + 1, dcap, mbf, mb, d_ur, d_dp, d_nm, st);
    if (rc) return rc;
    ORBX_HIP(hipMemcpyAsync(h->h_counts, h->d_counts, sizeof(int32_t) * 2, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipMemcpyAsync(h->h_kps, h->d_kps, sizeof(orbx_keypoint_t) * 2 * (size_t)dcap, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipMemcpyAsync(h->h_desc, h->d_desc, (size_t)32 * 2 * dcap, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipMemcpyAsync(h->h_sfr, h->d_sfr, sizeof(float) * (2 * (size_t)dcap + 4), hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    int status = ORBX_OK;
    int n0 = h->h_counts[0], n1 = h->h_counts[1];
    if (n0 > cap || n1 > cap) {
        orbx_set_error("stereo frame produced %d / %d keypoints, cap %d", n0, n1, cap);
        status = ORBX_ERR_CAPACITY;
        n0 = std::min(n0, cap); n1 = std::min(n1, cap);
    }
    *nl = n0; *nr = n1;
    if (n0 > 0) {
        memcpy(kl, h->h_kps, sizeof(orbx_keypoint_t) * n0);
        memcpy(dl, h->h_desc, (size_t)32 * n0);
        memcpy(uright, h->h_sfr, sizeof(float) * n0);
        memcpy(depth, h->h_sfr + dcap, sizeof(float) * n0);
    }
    if (n1 > 0) {
        memcpy(kr, h->h_kps + dcap, sizeof(orbx_keypoint_t) * n1);
        memcpy(dr, h->h_desc + (size_t)dcap * 32, (size_t)32 * n1);
    }
    if (nmatch) *nmatch = ((const int32_t *)(h->h_sfr + 2 * (size_t)dcap))[0];
    return status;
}

extern "C" int orbx_stereo_frame(orbx_extractor_t *h, const uint8_t *left, const uint8_t *right, int w, int hgt, int stride,
                                 float mbf, float mb, int cap, orbx_keypoint_t *kl, uint8_t *dl, int *nl, orbx_keypoint_t *kr,
                                 uint8_t *dr, int *nr, float *uright, float *depth, int *nmatch) {
    if (!h || !kl || !dl || !nl || !kr || !dr || !nr || !uright || !depth || cap < 1) {
        orbx_set_error("orbx_stereo_frame: bad arguments");
        return ORBX_ERR_ARG;
    }
    *nl = 0; *nr = 0;
    if (nmatch) *nmatch = 0;
    if (!left || !right || w <= 0 || hgt <= 0) return ORBX_OK;   // empty image (:1046-1047)
    if (stride < w) { orbx_set_error("stride < width"); return ORBX_ERR_ARG; }
    return stereo_frame_run(h, left, right, nullptr, w, hgt, stride, 0, mbf, mb, cap, kl, dl, nl, kr, dr, nr, uright, depth, nmatch);
}

int orbx_internal_stereo_frame_device(orbx_extractor *h, const uint8_t *d_pair, int w, int hgt, int stride, size_t img_bytes, float mbf,
                                      float mb, int cap, orbx_keypoint_t *kl, uint8_t *dl, int *nl, orbx_keypoint_t *kr, uint8_t *dr,
                                      int *nr, float *uright, float *depth, int *nmatch) {
    return stereo_frame_run(h, nullptr, nullptr, d_pair, w, hgt, stride, img_bytes, mbf, mb, cap, kl, dl, nl, kr, dr, nr, uright, depth,
                            nmatch);
}

// ---- the latency form: one stereo frame, no copy commands (include/orbx.h: orbx_stereo_frame_view)
extern "C" void *orbx_host_alloc(size_t bytes) {
    void *p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return p;
}
extern "C" void orbx_host_free(void *p) { if (p) (void)hipHostFree(p); }

// the address a kernel reads the image at, or NULL when the memory is ordinary pageable host memory
const uint8_t *orbx_internal_device_visible(const uint8_t *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    if (hipPointerGetAttributes(&a, p) != hipSuccess) { (void)hipGetLastError(); return nullptr; }   // (older runtimes: an error for unregistered memory)
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged) return (const uint8_t *)a.devicePointer;
    return nullptr;
}

extern "C" int orbx_stereo_frame_view(orbx_extractor_t *h, const uint8_t *left, const uint8_t *right, int w, int hgt, int stride,
                                      float mbf, float mb, orbx_stereo_view_t *view) {
    if (!h || !view) { orbx_set_error("orbx_stereo_frame_view: bad arguments"); return ORBX_ERR_ARG; }
    memset(view, 0, sizeof(*view));
    if (!left || !right || w <= 0 || hgt <= 0) return ORBX_OK;   // empty image (:1046-1047)
    if (stride < w) { orbx_set_error("stride < width"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    int rc = ensure_plan(h, w, hgt, 2);
    if (rc) return rc;
    const int cap = (h->sp.max_kp + 3) & ~3;   // the record's blocks are 16-byte aligned for any multiple of 4
    const size_t recBytes = (size_t)128 * cap + 16;
    if (h->fv_cap < cap) {
        ORBX_HIP(hipStreamSynchronize(h->stream));
        for (int i = 0; i < 2; i++) {
            hipFree(h->fv_d[i]); h->fv_d[i] = nullptr;
            if (h->fv_h[i]) { hipHostFree(h->fv_h[i]); h->fv_h[i] = nullptr; }
        }
        h->fv_cap = 0;
        for (int i = 0; i < 2; i++) {
            ORBX_HIP(scratch_malloc(&h->fv_d[i], recBytes));
            // on the handle's stream, in front of the call's kernels.  (hipMemset runs on the NULL stream and may return before it has run; the
            // handle's stream is non-blocking, so nothing ordered that memset against k_describe / k_stereo_finish: on a busy GPU it could zero a
            // record in HBM after they had written it - the pinned twin stayed right, the guided search on the HBM record found nothing.)
            ORBX_HIP(hipMemsetAsync(h->fv_d[i], 0, recBytes, h->stream));
            ORBX_HIP(scratch_host_malloc((void **)&h->fv_h[i], recBytes, hipHostMallocDefault));
            ORBX_HIP(hipHostGetDevicePointer((void **)&h->fv_hdev[i], h->fv_h[i], 0));
        }
        h->fv_cap = cap;
    }
    const size_t span = (size_t)stride * (hgt - 1) + w, img_bytes = (span + 255) & ~(size_t)255;
    const uint8_t *dl = orbx_internal_device_visible(left), *dr = orbx_internal_device_visible(right);
    if (!dl || !dr) {   // pageable memory: one memcpy per image into the handle's pinned staging buffer, read from there
        if (h->fv_stage_bytes < 2 * img_bytes) {
            ORBX_HIP(hipStreamSynchronize(h->stream));
            if (h->fv_stage) { hipHostFree(h->fv_stage); h->fv_stage = nullptr; h->fv_stage_bytes = 0; }
            ORBX_HIP(scratch_host_malloc((void **)&h->fv_stage, 2 * img_bytes, hipHostMallocDefault));
            ORBX_HIP(hipHostGetDevicePointer((void **)&h->fv_stage_dev, h->fv_stage, 0));
            h->fv_stage_bytes = 2 * img_bytes;
        }
        if (!dl) { memcpy(h->fv_stage, left, span); dl = h->fv_stage_dev; }
        if (!dr) { memcpy(h->fv_stage + img_bytes, right, span); dr = h->fv_stage_dev + img_bytes; }
    }
    const int i = h->fv_next;
    h->fv_next ^= 1;
    uint8_t *rec = h->fv_d[i];
    const size_t c = (size_t)cap;
    hipStream_t st = h->stream;
    // image b of the batch of two sits at dl + b * (dr - dl): the kernels add the (unsigned, possibly wrapped) difference once
    // the descriptor kernel stores every record twice - HBM and the pinned twin - unless an option took the split-call path (its scratch records move later)
    h->descHostDelta = h->opt[15] >= 2 ? 0 : (long long)((intptr_t)h->fv_hdev[i] - (intptr_t)rec);
    const long long twin = h->descHostDelta;
    rc = launch_pipeline(h, dl, 2, w, hgt, stride, (size_t)((uintptr_t)dr - (uintptr_t)dl), (orbx_keypoint_t *)rec, rec + 56 * c, (int32_t *)(rec + 128 * c), cap, st);
    h->descHostDelta = 0;
    if (rc) return rc;
    if (!h->fv_flag) {
        ORBX_HIP(scratch_host_malloc((void **)&h->fv_flag, 64, hipHostMallocMapped | hipHostMallocCoherent));
        *h->fv_flag = 0;
        ORBX_HIP(hipHostGetDevicePointer((void **)&h->fv_flag_dev, h->fv_flag, 0));
    }
    int armed = 0;
    const int seq = ++h->fv_seq;
    rc = orbx_internal_stereo_frame_record(h, rec, h->fv_hdev[i], cap, mbf, mb, st, twin != 0, h->opt[27] == 0 ? h->fv_flag_dev : nullptr, seq, &armed);
    if (rc) return rc;
    // The last kernel stores the call's number into the completion word behind the record; the host polls it (a stream synchronisation
    // adds 10-15 us of wake-up latency to a 120-us call) and falls back to the stream after a few milliseconds.  ORBX_OPT_STREAM_SYNC = 1: the stream wait.
    bool done = false;
    if (armed)
        for (int spin = 0; spin < 200000 && !done; spin++) {
            done = __atomic_load_n(h->fv_flag, __ATOMIC_ACQUIRE) == seq;
            if (!done) __builtin_ia32_pause();
        }
    if (!done) ORBX_HIP(hipStreamSynchronize(st));
    const uint8_t *hr = h->fv_h[i];
    const int32_t *tail = (const int32_t *)(hr + 128 * c);
    view->nl = std::min(tail[0], cap); view->nr = std::min(tail[1], cap); view->nmatch = tail[2]; view->cap = cap;
    view->kl = (const orbx_keypoint_t *)hr; view->kr = (const orbx_keypoint_t *)(hr + 28 * c);
    view->dl = hr + 56 * c; view->dr = hr + 88 * c;
    view->uright = (const float *)(hr + 120 * c); view->depth = (const float *)(hr + 124 * c);
    view->d_kl = (const orbx_keypoint_t *)rec; view->d_kr = (const orbx_keypoint_t *)(rec + 28 * c);
    view->d_dl = rec + 56 * c; view->d_dr = rec + 88 * c;
    view->d_uright = (const float *)(rec + 120 * c); view->d_depth = (const float *)(rec + 124 * c);
    return ORBX_OK;
}

extern "C" int orbx_extract(orbx_extractor_t *h, const uint8_t *img, int w, int hgt, int stride,
                            orbx_keypoint_t *kps, uint8_t *desc, int cap, int *n_out) {
    if (!h || !n_out) { orbx_set_error("orbx_extract: bad arguments"); return ORBX_ERR_ARG; }
    if (!img || w <= 0 || hgt <= 0) { *n_out = 0; return ORBX_OK; }  // empty image (:1046-1047)
    const uint8_t *imgs[1] = {img};
    return orbx_extract_batch(h, imgs, 1, w, hgt, stride, kps, desc, cap, n_out);
}

int orbx_internal_level(const orbx_extractor *h, int level, int *w, int *hgt, int *pstride,
                        unsigned long long *poff) {
    if (!h || level < 0 || level >= h->nlevels || h->pw == 0) return ORBX_ERR_ARG;
    const LevelGeom &g = h->sp.geom[level];
    *w = g.w; *hgt = g.h; *pstride = g.pstride; *poff = g.poff;
    return ORBX_OK;
}

// The layout of in-place input (include/orbx.h): level 0 of what plan_size decides for the size - nothing is restated here.  The feature
// budget only sizes the quad-tree's LDS, so the geometry (and every refusal that comes from it) is that of any handle with these levels.
extern "C" int orbx_level0_layout(int w, int hgt, int nlevels, float scale_factor, orbx_level0_layout_t *out) {
    if (!out || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !(scale_factor > 1.0f)) { orbx_set_error("orbx_level0_layout: bad arguments"); return ORBX_ERR_ARG; }
    SizeInput in = {};
    in.w = w; in.h = hgt; in.nlevels = nlevels; in.scale_factor = scale_factor;
    extractor_tables(1, in.scale_factor, nlevels, &in.tb);
    SizePlan sp;
    const int rc = plan_size(in, &sp);
    if (rc) return rc;
    const LevelGeom &g0 = sp.geom[0];
    out->pstride = g0.pstride; out->prows = g0.prows;
    out->pixel0_offset = g0.poff + (uint64_t)ORBX_EDGE * g0.pstride + ORBX_EDGE;
    out->image_bytes = level0_image_bytes(g0);
    return ORBX_OK;
}

// Level 0 of the last batch copied from the caller's images into the pyramid block (with its frame), for callers that look at the
// padded buffers after a call that read it in place.  The kernels go on reading it in place: h->lv0 stays.
static int ensure_level0(orbx_extractor *h) {
    if (h->lv0Stale <= 0 || !h->lv0.base) return ORBX_OK;
    const LevelGeom &g0 = h->sp.geom[0];
    (void)hipGetLastError();
    launch_pad0(h, h->lv0.base + (size_t)ORBX_EDGE * g0.pstride + ORBX_EDGE, h->d_pyr, h->lv0Stale, g0.pstride, h->lv0.imgBytes, h->last_stream);
    ORBX_HIP(hipGetLastError());
    h->lv0Stale = 0;
    return ORBX_OK;
}

// copyMakeBorder of the levels >= 1 of the last batch, for callers that look at the padded buffers
static int ensure_frames(orbx_extractor *h) {
    if (h->framesStale <= 0) return ORBX_OK;
    const int nl = h->nlevels, B = h->framesStale;
    hipStream_t st = h->last_stream;
    const LevelGeom &g1 = h->sp.geom[1];
    const int p1 = (g1.w + 2 * ORBX_EDGE + 3) >> 2, tot1 = 2 * ORBX_EDGE * p1 + g1.h * 12;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_pyr_pad<false>, dim3((tot1 + 255) / 256, nl - 1, B), dim3(256), 0, st, (const uint8_t *)nullptr, 0, (size_t)0,
                       h->d_pyr, h->sp.pyrImgBytes, h->d_geom, 1);
    ORBX_HIP(hipGetLastError());
    h->framesStale = 0;
    return ORBX_OK;
}

extern "C" int orbx_pyramid_device(orbx_extractor_t *h, int b, int level, const uint8_t **d_ptr, int *w, int *hgt,
                                   int *stride) {
    if (!h || !d_ptr || level < 0 || level >= h->nlevels || h->pw == 0 || b < 0 || b >= h->pB) {
        orbx_set_error("orbx_pyramid_device: bad arguments or no frame extracted yet");
        return ORBX_ERR_ARG;
    }
    if (level > 0) {   // the caller may walk into the 19-px frame around the ROI, as with the reference's padded cv::Mat
        ORBX_HIP(hipSetDevice(h->device));
        const int rc = ensure_frames(h);
        if (rc) return rc;
    } else {           // level 0 of a call that read the caller's images in place: copied into the pyramid block now
        ORBX_HIP(hipSetDevice(h->device));
        const int rc = ensure_level0(h);
        if (rc) return rc;
    }
    const LevelGeom &g = h->sp.geom[level];
    *d_ptr = h->d_pyr + (size_t)b * h->sp.pyrImgBytes + g.poff + (size_t)ORBX_EDGE * g.pstride + ORBX_EDGE;
    if (w) *w = g.w;
    if (hgt) *hgt = g.h;
    if (stride) *stride = g.pstride;
    return ORBX_OK;
}

extern "C" int orbx_pyramid_host(orbx_extractor_t *h, int b, int level, int padded, uint8_t *dst, int dst_stride,
                                 int *w, int *hgt) {
    if (!h || level < 0 || level >= h->nlevels || h->pw == 0 || b < 0 || b >= h->pB) {
        orbx_set_error("orbx_pyramid_host: bad arguments or no frame extracted yet");
        return ORBX_ERR_ARG;
    }
    const LevelGeom &g = h->sp.geom[level];
    const int ow = padded ? g.w + 2 * ORBX_EDGE : g.w, oh = padded ? g.h + 2 * ORBX_EDGE : g.h;
    if (w) *w = ow;
    if (hgt) *hgt = oh;
    if (!dst) return ORBX_OK;
    if (dst_stride < ow) { orbx_set_error("dst_stride < width"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    if (padded && level > 0) { const int rc = ensure_frames(h); if (rc) return rc; }
    if (level == 0) { const int rc = ensure_level0(h); if (rc) return rc; }
    if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
    const uint8_t *src = h->d_pyr + (size_t)b * h->sp.pyrImgBytes + g.poff +
                         (padded ? 0 : (size_t)ORBX_EDGE * g.pstride + ORBX_EDGE);
    // linear device-to-host copy of the row span, rows unpacked on the host (2-D copies of odd widths are very slow)
    const size_t span = (size_t)g.pstride * (oh - 1) + ow;
    static thread_local std::vector<uint8_t> tmp;
    if (tmp.size() < span) tmp.resize(span);
    ORBX_HIP(hipMemcpy(tmp.data(), src, span, hipMemcpyDeviceToHost));
    for (int r = 0; r < oh; r++) memcpy(dst + (size_t)r * dst_stride, tmp.data() + (size_t)r * g.pstride, ow);
    return ORBX_OK;
}

extern "C" int orbx_level_counts(orbx_extractor_t *h, int b, int32_t *candidates, int32_t *keypoints) {
    if (!h || h->pw == 0 || b < 0 || b >= h->pB || !h->last_valid) { orbx_set_error("orbx_level_counts: bad arguments or no frame extracted yet"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    ORBX_HIP(hipStreamSynchronize(h->last_stream));
    if (candidates) ORBX_HIP(hipMemcpy(candidates, h->d_candCnt + (size_t)b * h->nlevels, sizeof(int32_t) * h->nlevels, hipMemcpyDeviceToHost));
    if (keypoints) ORBX_HIP(hipMemcpy(keypoints, h->d_lvlCnt + (size_t)b * h->nlevels, sizeof(int32_t) * h->nlevels, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

#ifdef ORBX_DEVELOPER   // ---- read-only stage hooks: developer build only (include/orbx_dev.h)
// the compacted key arrays of the last call, when k_octree_pyr read the cell lists in place: gathered now, for the test hooks
static int ensure_cand(orbx_extractor *h) {
    if (h->candStale <= 0) return ORBX_OK;
    const int nl = h->nlevels, B = h->candStale;
    CellBases cb;
    for (int l = 0; l <= ORBX_MAX_LEVELS; l++) cb.v[l] = l < nl ? h->sp.geom[l].cellBase : h->sp.totalCells;
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_gather, dim3((h->sp.totalCells + GATHER_CELLS_PER_BLOCK - 1) / GATHER_CELLS_PER_BLOCK, B), dim3(256), 0, h->last_stream,
                       h->d_geom, nl, h->sp.totalCells, h->d_cellCnt, h->d_cellRaw, h->d_slots, h->sp.slotsPerImg, h->d_cand, h->sp.keysPerImg,
                       h->d_candCnt, h->ini_th, h->min_th, cb, (int32_t *)nullptr, 0, (int32_t *)nullptr, 0);
    ORBX_HIP(hipGetLastError());
    h->candStale = 0;
    return ORBX_OK;
}

// test / probe hook: which (image, level)s of the last call took the exact form of the quad-tree because the count pyramid was too shallow
extern "C" int orbx_debug_octree_fallbacks(orbx_extractor_t *h, int32_t *out, int n) {
    if (!h || !out || n < 1 || h->pw == 0 || n > h->pB * h->nlevels) { orbx_set_error("orbx_debug_octree_fallbacks: bad arguments"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
    ORBX_HIP(hipMemcpy(out, h->d_octFallback, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

extern "C" int orbx_debug_level_points(orbx_extractor_t *h, int b, int level, int stage, int32_t *out, int cap,
                                       int *n_out) {
    if (!h || !n_out || level < 0 || level >= h->nlevels || h->pw == 0 || b < 0 || b >= h->pB || stage < 0 || stage > 1) {
        orbx_set_error("orbx_debug_level_points: bad arguments");
        return ORBX_ERR_ARG;
    }
    ORBX_HIP(hipSetDevice(h->device));
    if (stage == 0) { const int rc = ensure_cand(h); if (rc) return rc; }
    if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
    const LevelGeom &g = h->sp.geom[level];
    int32_t n = 0;
    const int32_t *cntp = (stage == 0 ? h->d_candCnt : h->d_lvlCnt) + b * h->nlevels + level;
    ORBX_HIP(hipMemcpy(&n, cntp, sizeof(int32_t), hipMemcpyDeviceToHost));
    *n_out = n;
    if (!out || n == 0) return ORBX_OK;
    const int m = std::min(n, cap);
    std::vector<uint32_t> tmp(m);
    const uint32_t *src = stage == 0 ? h->d_cand + (size_t)b * h->sp.keysPerImg + g.keyOff
                                     : h->d_lvlKp + (size_t)b * h->sp.lvlKpCap + g.lvlKpOff;
    ORBX_HIP(hipMemcpy(tmp.data(), src, sizeof(uint32_t) * m, hipMemcpyDeviceToHost));
    for (int i = 0; i < m; i++) {
        out[3 * i] = (int32_t)(tmp[i] & 0xFFF);
        out[3 * i + 1] = (int32_t)((tmp[i] >> 12) & 0xFFF);
        out[3 * i + 2] = (int32_t)(tmp[i] >> 24);
    }
    return n > cap ? ORBX_ERR_CAPACITY : ORBX_OK;
}

#endif   // ORBX_DEVELOPER

// Which FAST kernel(s) a batch of B images of the planned size runs (the rule of launch_pipeline): for benchmarks that name the
// kernel they time.  *strips = 1 if k_fast_strips takes part, *cells = 1 if k_fast_cells does.
extern "C" int orbx_fast_kernels(const orbx_extractor_t *h, int B, int *strips, int *cells, int *images_per_launch) {
    if (!h || h->pw == 0 || B < 1) { orbx_set_error("orbx_fast_kernels: no plan yet"); return ORBX_ERR_ARG; }
    // the last call's own chunk count when it was a batch of this size (it knows whether its pyramid was built ahead), else the rule
    const int nch = (h->last_valid && h->lastB == B) ? h->lastChunks : chunk_count(h->opt, B, h->profiling == 1, false);
    B = B / nch;                                   // the first chunk is the one whose FAST stage carries the events
    if (images_per_launch) *images_per_launch = B;
    ChunkPlan p;
    const int rc = plan_chunk(plan_input(h, B, nch, h->profiling == 1, h->profiling != 0, false, false), &p);
    if (rc) return rc;
    if (strips) *strips = p.strips;
    if (cells) *cells = p.fastCells;
    return ORBX_OK;
}

#ifdef ORBX_DEVELOPER
// The launch rule by itself (no HIP call, no handle): PlanInput in, ChunkPlan out, both as flat int32 arrays (include/orbx_dev.h).
static_assert(ORBX_DEBUG_SIZE_PLAN_INTS == 31 + ORBX_MAX_LEVELS + 1 + 2 * 8 * (int)(sizeof(ChainPlan) / sizeof(int)), "include/orbx_dev.h and orbx_size_plan.h disagree");
static_assert(ORBX_DEBUG_PYR_RECORDS_INTS == 2 + 6 * ORBX_MAX_LEVELS && sizeof(PyrColRec) == 16, "include/orbx_dev_pyr.h and orbx_size_plan.h disagree");
static_assert(ORBX_DEBUG_PLAN_INPUT_INTS == ORBX_PLAN_INPUT_INTS && ORBX_DEBUG_CHUNK_PLAN_INTS == ORBX_CHUNK_PLAN_INTS, "include/orbx_dev.h and orbx_plan.h disagree");
extern "C" int orbx_debug_plan_chunk(const int32_t *in, int n_in, int32_t *out, int n_out) {
    PlanInput pi;
    if (!in || !out || n_in != ORBX_PLAN_INPUT_INTS || n_out != ORBX_CHUNK_PLAN_INTS) { orbx_set_error("orbx_debug_plan_chunk: bad arguments"); return ORBX_ERR_ARG; }
    memcpy(&pi, in, sizeof(pi));
    if (pi.B < 1 || pi.nl < 1 || pi.nl > ORBX_MAX_LEVELS) { orbx_set_error("orbx_debug_plan_chunk: bad B or nl"); return ORBX_ERR_ARG; }
    ChunkPlan p;
    const int rc = plan_chunk(pi, &p);
    if (rc == ORBX_OK) memcpy(out, &p, sizeof(p));
    return rc;
}
// What an image size decides, by itself (no HIP call, no handle): the tables of orbx_create, then plan_size (include/orbx_dev.h)
extern "C" int orbx_debug_size_plan(int nfeatures, float scale_factor, int nlevels, int w, int hgt, int pyr_tile, float *tables, int32_t *nfeat_umax,
                                    uint8_t *geom, int geom_bytes, int32_t *tab, int tab_cap, int64_t *scalars, int n_scalars) {
    if (!tables || !nfeat_umax || !geom || geom_bytes != (int)sizeof(LevelGeom) * ORBX_MAX_LEVELS || !scalars || n_scalars != ORBX_DEBUG_SIZE_PLAN_INTS ||
        (tab_cap > 0 && !tab) || nfeatures < 1 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !(scale_factor > 1.0f) || pyr_tile < 0 || pyr_tile > 64) {
        orbx_set_error("orbx_debug_size_plan: bad arguments");
        return ORBX_ERR_ARG;
    }
    SizeInput in = {};
    in.w = w; in.h = hgt; in.nlevels = nlevels; in.scale_factor = scale_factor; in.pyrTile = pyr_tile;
    extractor_tables(nfeatures, in.scale_factor, nlevels, &in.tb);
    memcpy(tables, in.tb.sf, sizeof(float) * 4 * ORBX_MAX_LEVELS);        // sf | isf | sig2 | isig2
    memcpy(nfeat_umax, in.tb.nfeat, sizeof(int32_t) * (ORBX_MAX_LEVELS + 16));   // nfeat | umax
    SizePlan sp;
    const int rc = plan_size(in, &sp);
    if (rc) return rc;
    memcpy(geom, sp.geom, sizeof(sp.geom));
    if (tab_cap > 0) memcpy(tab, sp.tab.data(), sizeof(int32_t) * std::min((size_t)tab_cap, sp.tab.size()));
    const int64_t v[31] = {sp.max_kp, sp.totalCells, sp.maxNodeCap, sp.lvlKpCap, (int64_t)sp.pyrImgBytes, (int64_t)sp.slotsPerImg, (int64_t)sp.keysPerImg,
                           sp.fastTileStride, sp.fastScoreStride, sp.fastTileRows, sp.fastLdsPerWave, sp.totalStrips, sp.stripLevels,
                           (int64_t)sp.octLdsBytes, (int64_t)sp.octPyrLdsBytes, sp.octPyrWords, sp.octBigMask, sp.octDeepMax, sp.octSliceStride, sp.histStride,
                           sp.pyrTilesX, sp.pyrTilesY, sp.pyrXSpanOff, sp.pyrYSpanOff, sp.pyrBufBytes, sp.pyrMaxDim, sp.pyrMaxPar, (int64_t)sp.pyrLdsBytes,
                           sp.nChains[0], sp.nChains[1], (int64_t)sp.tab.size()};
    int64_t *o = std::copy(v, v + 31, scalars);
    o = std::copy(sp.stripBase, sp.stripBase + ORBX_MAX_LEVELS + 1, o);
    std::copy((const int *)sp.chains, (const int *)sp.chains + 2 * 8 * 8, o);
    return ORBX_OK;
}
// k_pyr_level's records (include/orbx_dev_pyr.h): h == NULL what plan_pyr_records builds for the size, by itself; h != NULL what the handle's
// device buffers hold for its planned size
extern "C" int orbx_debug_pyr_records(orbx_extractor_t *h, int nfeatures, float scale_factor, int nlevels, int w, int hgt, uint32_t *cols, int cols_cap,
                                      uint32_t *bands, int bands_cap, int32_t *index, int n_index) {
    if (!index || n_index != ORBX_DEBUG_PYR_RECORDS_INTS || cols_cap < 0 || bands_cap < 0 || (cols_cap > 0 && !cols) || (bands_cap > 0 && !bands)) {
        orbx_set_error("orbx_debug_pyr_records: bad arguments");
        return ORBX_ERR_ARG;
    }
    PyrRecords built;
    const PyrRecords *pr = &built;
    if (h) {
        if (h->pw == 0) { orbx_set_error("orbx_debug_pyr_records: the handle has no plan yet"); return ORBX_ERR_ARG; }
        pr = &h->pr;
    } else {
        if (nfeatures < 1 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS || !(scale_factor > 1.0f)) { orbx_set_error("orbx_debug_pyr_records: bad arguments"); return ORBX_ERR_ARG; }
        SizeInput in = {};
        in.w = w; in.h = hgt; in.nlevels = nlevels; in.scale_factor = scale_factor;
        extractor_tables(nfeatures, in.scale_factor, nlevels, &in.tb);
        SizePlan sp;
        const int rc = plan_size(in, &sp);
        if (rc) return rc;
        plan_pyr_records(in, sp, &built);
    }
    const size_t colWords = pr->cols.size() * 4, bandWords = pr->bands.size();
    const size_t nc = std::min((size_t)cols_cap, colWords), nb = std::min((size_t)bands_cap, bandWords);
    if (h) {
        ORBX_HIP(hipSetDevice(h->device));
        if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
        if (nc) ORBX_HIP(hipMemcpy(cols, h->d_pyrCols, sizeof(uint32_t) * nc, hipMemcpyDeviceToHost));
        if (nb) ORBX_HIP(hipMemcpy(bands, h->d_pyrBands, sizeof(uint32_t) * nb, hipMemcpyDeviceToHost));
    } else {
        if (nc) memcpy(cols, pr->cols.data(), sizeof(uint32_t) * nc);
        if (nb) memcpy(bands, pr->bands.data(), sizeof(uint32_t) * nb);
    }
    int32_t *o = index;
    *o++ = (int32_t)colWords; *o++ = (int32_t)bandWords;
    o = std::copy(pr->nxc, pr->nxc + ORBX_MAX_LEVELS, o);
    o = std::copy(pr->colOff, pr->colOff + ORBX_MAX_LEVELS, o);
    o = std::copy(pr->nbands[0], pr->nbands[0] + 2 * ORBX_MAX_LEVELS, o);
    std::copy(pr->bandOff[0], pr->bandOff[0] + 2 * ORBX_MAX_LEVELS, o);
    return ORBX_OK;
}
// the plan chunk 0 of the handle's last extraction call executed
extern "C" int orbx_debug_last_plan(const orbx_extractor_t *h, int32_t *out, int n_out) {
    if (!h || !out || n_out != ORBX_CHUNK_PLAN_INTS || !h->last_valid) { orbx_set_error("orbx_debug_last_plan: bad arguments or no call yet"); return ORBX_ERR_ARG; }
    memcpy(out, &h->lastPlan, sizeof(h->lastPlan));
    return ORBX_OK;
}
// which form the handle's last extraction call ran (include/orbx_dev_level0.h): 1 = level 0 read in place, 0 = copied into the pyramid block
extern "C" int orbx_debug_level0_in_place(const orbx_extractor_t *h) {
    if (!h || !h->last_valid) { orbx_set_error("orbx_debug_level0_in_place: bad arguments or no call yet"); return ORBX_ERR_ARG; }
    return h->lv0.base != nullptr ? 1 : 0;
}
#endif

#ifdef ORBX_DEVELOPER
// Test hook for SURVEY section 8 row a8 (cv::GaussianBlur 7x7, sigma 2, fused into k_describe and never stored): the next
// single-image orbx_extract calls also write, for keypoint i, the 37x37 blurred block centred on it (the only blurred
// pixels the descriptor can read) to a device buffer, fetched here.  enable = 0 frees the buffer.
extern "C" int orbx_debug_blur_patches(orbx_extractor_t *h, int enable, uint8_t *out, int n) {
    if (!h) return ORBX_ERR_ARG;
    ORBX_HIP(hipSetDevice(h->device));
    if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
    if (out && n > 0) {
        if (!h->d_dbgBlur || n > h->dbgBlurCap) { orbx_set_error("orbx_debug_blur_patches: not enabled or n too large"); return ORBX_ERR_ARG; }
        ORBX_HIP(hipMemcpy(out, h->d_dbgBlur, (size_t)n * 37 * 37, hipMemcpyDeviceToHost));
        return ORBX_OK;
    }
    hipFree(h->d_dbgBlur); h->d_dbgBlur = nullptr; h->dbgBlurCap = 0;
    if (enable) {
        h->dbgBlurCap = h->sp.max_kp > 0 ? h->sp.max_kp + 300 : h->nfeatures + 3 * h->nlevels + 300;
        ORBX_HIP(scratch_malloc(&h->d_dbgBlur, (size_t)h->dbgBlurCap * 37 * 37));
    }
    return ORBX_OK;
}

// Test hook: level `level` of image b as k_blur_levels left it in the last call (inner ROI), and the mask of levels that were
// blurred as a whole (bit l).  A level outside the mask was blurred per keypoint inside k_describe: ORBX_ERR_ARG for it.
extern "C" int orbx_debug_blurred_level(orbx_extractor_t *h, int b, int level, uint8_t *dst, int dst_stride, unsigned *mask_out) {
    if (!h || h->pw == 0 || b < 0 || b >= h->pB) { orbx_set_error("orbx_debug_blurred_level: bad arguments"); return ORBX_ERR_ARG; }
    if (mask_out) *mask_out = h->blurMaskLast;
    if (!dst) return ORBX_OK;
    if (level < 0 || level >= h->nlevels || !((h->blurMaskLast >> level) & 1u) || !h->d_blur) {
        orbx_set_error("orbx_debug_blurred_level: level %d was not blurred as a whole (mask 0x%x)", level, h->blurMaskLast);
        return ORBX_ERR_ARG;
    }
    const LevelGeom &g = h->sp.geom[level];
    if (dst_stride < g.w) { orbx_set_error("dst_stride < width"); return ORBX_ERR_ARG; }
    ORBX_HIP(hipSetDevice(h->device));
    if (h->last_valid) ORBX_HIP(hipStreamSynchronize(h->last_stream));
    const uint8_t *src = h->d_blur + (size_t)b * h->sp.pyrImgBytes + g.poff + (size_t)ORBX_EDGE * g.pstride + ORBX_EDGE;
    const size_t span = (size_t)g.pstride * (g.h - 1) + g.w;
    std::vector<uint8_t> tmp(span);
    ORBX_HIP(hipMemcpy(tmp.data(), src, span, hipMemcpyDeviceToHost));
    for (int r = 0; r < g.h; r++) memcpy(dst + (size_t)r * dst_stride, tmp.data() + (size_t)r * g.pstride, g.w);
    return ORBX_OK;
}

#endif   // ORBX_DEVELOPER

extern "C" int orbx_set_profiling(orbx_extractor_t *h, int enabled) {
    if (!h) return ORBX_ERR_ARG;
    ORBX_HIP(hipSetDevice(h->device));
    for (int r = 0; r < ORBX_EV_RING; r++)
        if (h->ev_pending[r]) { ORBX_HIP(hipEventSynchronize(h->ev[r][h->ev_pending[r] == 2 ? 2 : 4])); h->ev_pending[r] = 0; }
    if (enabled < 0 || enabled > 3) { orbx_set_error("orbx_set_profiling: mode %d", enabled); return ORBX_ERR_ARG; }
    h->profiling = enabled;
    if (enabled) {   // the ordering kernel in front of the FAST bracket: its first launch loads code, keep that out of the timed calls
        hipLaunchKernelGGL(k_nop, dim3(1), dim3(64), 0, h->stream);
        ORBX_HIP(hipStreamSynchronize(h->stream));
    }
    h->prof_calls = 0;
    h->ev_head = 0;
    h->acc_n = 0;
    for (int i = 0; i < ORBX_NUM_STAGES; i++) h->acc_ms[i] = 0;
    return ORBX_OK;
}
extern "C" int orbx_get_stage_ms(orbx_extractor_t *h, float *ms, int *ncalls) {
    if (!h || !ms) return ORBX_ERR_ARG;
    ORBX_HIP(hipSetDevice(h->device));
    for (int r = 0; r < ORBX_EV_RING; r++)
        if (h->ev_pending[r]) { int rc = harvest_events(h, r); if (rc) return rc; }
    if (h->acc_n == 0) { orbx_set_error("no profiled batch recorded"); return ORBX_ERR_ARG; }
    for (int i = 0; i < ORBX_NUM_STAGES; i++) ms[i] = (float)(h->acc_ms[i] / (double)h->acc_n);
    if (ncalls) *ncalls = (int)h->acc_n;
    return ORBX_OK;
}
