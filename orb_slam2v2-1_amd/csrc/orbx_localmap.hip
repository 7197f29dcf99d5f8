// orbx_localmap.hip — the local map on the device (row a34, prefix orbt_): Tracking::UpdateLocalMap (reference: src/Tracking.cc:1340-1484)
// over a snapshot of the map that stays resident between frames.  The kernels' bodies are in orbx_localmap_dev.h, which
// tests/cpp/localmap_lockstep.cc compiles for the host; here are the kernels around them and the host side: the handle, the checks, the
// packing of the snapshot and the launches of a frame.  DESIGN.md section 6, "k_lm_*".
#include "orbx_internal.h"
#include "orbx_stage_plan.h"
#include "orbx_localmap_dev.h"

static_assert(sizeof(orbt_pointview_t) == 24 && sizeof(orbm_worldpoint_t) == 40 && sizeof(orbt_local_info_t) == 32 && sizeof(LmHead) == 32,
              "record sizes of include/orbx.h");
#define LM_GRID 256   // the fixed grid of the kernels over the walk: they read its length from device memory and stride

// One workgroup.  K <= ORBC_LDS_KEYFRAMES: the counters live in LDS and every entry of the row is stored at the end; beyond: the adds go
// to the row itself, which the call zeroed in its own stream
__global__ __launch_bounds__(COV_COUNT_THREADS) void k_lm_vote(LmMap M, LmFrame F) {
    __shared__ int32_t tab[ORBC_LDS_KEYFRAMES];
    const int K = M.T.K;
    const bool lds = K <= ORBC_LDS_KEYFRAMES;
    if (lds) {
        for (int k = threadIdx.x; k < K; k += COV_COUNT_THREADS) tab[k] = 0;
        __syncthreads();
    }
    lm_vote(M, F, lds ? tab : F.counters);
    if (lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < K; k += COV_COUNT_THREADS) F.counters[k] = tab[k];
    }
}
__global__ __launch_bounds__(LM_KF_THREADS) void k_lm_keyframes(LmMap M, LmFrame F) {
    __shared__ uint32_t bits[ORBC_MAX_CULL_KEYFRAMES / 32];
    __shared__ unsigned long long sBest;
    __shared__ int sWave[LM_KF_THREADS / COV_WAVE], sScan[LM_KF_THREADS], sAny, sLen, sEnd;
    lm_keyframes(M, F, bits, sWave, sScan, &sAny, &sLen, &sEnd, &sBest);
}
__global__ __launch_bounds__(LM_THREADS) void k_lm_first(LmMap M, LmFrame F) { lm_first(M, F); }
__global__ __launch_bounds__(LM_THREADS) void k_lm_count(LmMap M, LmFrame F) {
    __shared__ int sWave[LM_THREADS / COV_WAVE];
    lm_count(M, F, sWave);
}
__global__ __launch_bounds__(LM_THREADS) void k_lm_scan(LmFrame F) {
    __shared__ int sScan[LM_THREADS];
    lm_scan(F, sScan);
}
__global__ __launch_bounds__(LM_THREADS) void k_lm_emit(LmMap M, LmFrame F) {
    __shared__ int sWave[LM_THREADS / COV_WAVE];
    lm_emit(M, F, sWave);
}
__global__ __launch_bounds__(LM_THREADS) void k_lm_holder(LmMap M, LmFrame F) { lm_holder(M, F); }
__global__ __launch_bounds__(LM_THREADS) void k_lm_clean(LmMap M, LmFrame F) { lm_clean(M, F); }

// ---------------------------------------------------------------- host side
struct orbt_localmap {
    int device = 0;
    hipStream_t stream = nullptr;
    // the last map whose host checks passed, and whether it reached the device
    int K = 0, P = 0; long long F = 0; size_t snapBytes = 0; bool hasShape = false, resident = false; int mapStatus = ORBX_ERR_ARG;
    uint8_t *d_map = nullptr, *h_map = nullptr; size_t mapCap = 0, mapHostCap = 0;   // the snapshot and its pinned mirror
    uint8_t *d_state = nullptr; size_t stateCap = 0; bool dirty = false;   // first [stateCap] | inframe [stateCap], idle between calls
    uint8_t *d_frame = nullptr, *h_frame = nullptr; size_t frameCap = 0, frameHostCap = 0;   // a frame's block; the mirror ends with the outputs
    LmMap M;
    size_t devBytes = 0;
};

static int lm_fail(const char *fn, const char *what, long long at, long long v) {
    orbx_set_error("%s: %s (at %lld: %lld)", fn, what, at, v);
    return ORBX_ERR_ARG;
}
// off[0..n]: starts at 0 and does not decrease; the entries of ids[0..off[n]) are slots
static int lm_check_lists(const char *fn, const char *name, const int32_t *off, const int32_t *ids, int n, int K) {
    char what[96];
    if (!off) { orbx_set_error("%s: %s_off is NULL", fn, name); return ORBX_ERR_ARG; }
    if (off[0] != 0) { snprintf(what, sizeof what, "%s_off does not start at 0", name); return lm_fail(fn, what, 0, off[0]); }
    for (int k = 0; k < n; k++)
        if (off[k + 1] < off[k]) { snprintf(what, sizeof what, "%s_off decreases", name); return lm_fail(fn, what, k + 1, off[k + 1]); }
    if (off[n] > 0 && !ids) { orbx_set_error("%s: %s is NULL", fn, name); return ORBX_ERR_ARG; }
    for (int i = 0; i < off[n]; i++)
        if (ids[i] < 0 || ids[i] >= K) { snprintf(what, sizeof what, "%s slot out of range", name); return lm_fail(fn, what, i, ids[i]); }
    return ORBX_OK;
}

// grow-only device block (+ pinned mirror of hostNeed bytes when h is given)
static int lm_reserve(orbt_localmap *h, uint8_t **d, size_t *cap, size_t need, uint8_t **hp, size_t *hcap, size_t hostNeed) {
    if (need > *cap) {
        if (*d) { ORBX_HIP(hipFree(*d)); h->devBytes -= *cap; *d = nullptr; *cap = 0; }
        const size_t c = need * 2 > ((size_t)1 << 16) ? need * 2 : ((size_t)1 << 16);
        ORBX_HIP(scratch_malloc(d, c));
        *cap = c; h->devBytes += c;
    }
    if (hp && hostNeed > *hcap) {
        if (*hp) { ORBX_HIP(hipHostFree(*hp)); *hp = nullptr; *hcap = 0; }
        const size_t c = hostNeed * 2 > ((size_t)1 << 16) ? hostNeed * 2 : ((size_t)1 << 16);
        ORBX_HIP(scratch_host_malloc((void **)hp, c, hipHostMallocDefault));
        *hcap = c;
    }
    return ORBX_OK;
}
static int lm_device(orbt_localmap *h) {
    ORBX_HIP(hipSetDevice(h->device));
    if (!h->stream) ORBX_HIP(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
    return ORBX_OK;
}
// first [cap] = LM_IDLE, inframe [cap] = 0: at allocation, and after a call that did not reach its cleaning pass
static int lm_state_idle(orbt_localmap *h) {
    ORBX_HIP(hipMemsetD32Async((hipDeviceptr_t)h->d_state, LM_IDLE, h->stateCap, h->stream));
    ORBX_HIP(hipMemsetAsync(h->d_state + h->stateCap * 4, 0, h->stateCap, h->stream));
    h->dirty = false;
    return ORBX_OK;
}
static int lm_state_reserve(orbt_localmap *h, size_t P) {
    if (P > h->stateCap) {
        if (h->d_state) { ORBX_HIP(hipFree(h->d_state)); h->devBytes -= h->stateCap * 5; h->d_state = nullptr; h->stateCap = 0; }
        const size_t c = stage_align(P * 2 > 4096 ? P * 2 : 4096);
        ORBX_HIP(scratch_malloc(&h->d_state, c * 5));
        h->stateCap = c; h->devBytes += c * 5;
        return lm_state_idle(h);
    }
    return h->dirty ? lm_state_idle(h) : ORBX_OK;
}

// the device, the snapshot block with its mirror and the state for P points; nothing of an earlier frame still runs on return
static int lm_map_reserve(orbt_localmap *h, size_t need, size_t P) {
    int rc = lm_device(h);
    if (rc) return rc;
    ORBX_HIP(hipStreamSynchronize(h->stream));
    rc = lm_reserve(h, &h->d_map, &h->mapCap, need, &h->h_map, &h->mapHostCap, need);
    return rc ? rc : lm_state_reserve(h, P);
}
// the ONE upload of a snapshot; the mirror is free again on return
static int lm_map_upload(orbt_localmap *h, size_t bytes) {
    ORBX_HIP(hipMemcpyAsync(h->d_map, h->h_map, bytes, hipMemcpyHostToDevice, h->stream));
    ORBX_HIP(hipStreamSynchronize(h->stream));
    return ORBX_OK;
}

extern "C" int orbt_localmap_create(int device, orbt_localmap_t **out) {
    if (!out) { orbx_set_error("orbt_localmap_create: NULL out"); return ORBX_ERR_ARG; }
    *out = nullptr;
    if (device < 0) { orbx_set_error("orbt_localmap_create: bad device %d", device); return ORBX_ERR_ARG; }
    orbt_localmap *h = new (std::nothrow) orbt_localmap();
    if (!h) { orbx_set_error("orbt_localmap_create: out of memory"); return ORBX_ERR_ARG; }
    h->device = device;
    *out = h;
    return ORBX_OK;
}

extern "C" void orbt_localmap_destroy(orbt_localmap_t *h) {
    if (!h) return;
    if (h->stream || h->d_map || h->h_map || h->d_state || h->d_frame || h->h_frame) {
        hipSetDevice(h->device);
        if (h->stream) { hipStreamSynchronize(h->stream); hipStreamDestroy(h->stream); }
        hipFree(h->d_map); hipFree(h->d_state); hipFree(h->d_frame);
        if (h->h_map) hipHostFree(h->h_map);
        if (h->h_frame) hipHostFree(h->h_frame);
    }
    delete h;
}

extern "C" int orbt_localmap_info(const orbt_localmap_t *h, int *K, int *P, int64_t *features, size_t *snapshot_bytes, size_t *device_bytes) {
    if (!h) { orbx_set_error("orbt_localmap_info: NULL handle"); return ORBX_ERR_ARG; }
    if (K) *K = h->K;
    if (P) *P = h->P;
    if (features) *features = h->F;
    if (snapshot_bytes) *snapshot_bytes = h->snapBytes;
    if (device_bytes) *device_bytes = h->devBytes;
    return ORBX_OK;
}

extern "C" int orbt_localmap_set_map(orbt_localmap_t *h, const orbt_map_t *map) {
    const char *fn = "orbt_localmap_set_map";
    if (!h || !map) { orbx_set_error("%s: NULL handle or map", fn); return ORBX_ERR_ARG; }
    int rc = orbx_internal_cov_check_table(fn, map->table);
    if (rc) return rc;
    const orbc_table_t *t = map->table;
    const int K = t->K, P = t->P;
    const orbc_queries_t *q = map->features;
    if (!q || q->Q != K) return lm_fail(fn, "features: one query per keyframe, Q == K", 0, q ? q->Q : -1);
    rc = orbx_internal_cov_check_queries(fn, t, q, false);
    if (rc) return rc;
    for (int k = 0; k < K; k++)
        if (q->query_kf[k] != k) return lm_fail(fn, "features: query_kf[q] is not q", k, q->query_kf[k]);
    if (K > 0 && !map->parent) { orbx_set_error("%s: parent is NULL", fn); return ORBX_ERR_ARG; }
    for (int k = 0; k < K; k++)
        if (map->parent[k] < -1 || map->parent[k] >= K) return lm_fail(fn, "parent out of range", k, map->parent[k]);
    rc = lm_check_lists(fn, "cov", map->cov_off, map->cov, K, K);
    if (rc) return rc;
    rc = lm_check_lists(fn, "child", map->child_off, map->child, K, K);
    if (rc) return rc;
    if (P > 0 && (!map->views || !map->desc)) { orbx_set_error("%s: views or desc is NULL", fn); return ORBX_ERR_ARG; }
    if (K > ORBC_MAX_CULL_KEYFRAMES) { orbx_set_error("%s: %d keyframes, at most %d", fn, K, ORBC_MAX_CULL_KEYFRAMES); return ORBX_ERR_UNSUPPORTED; }
    const long long nfeat = K > 0 ? q->feat_off[K] : 0;
    if (nfeat < 0 || nfeat >= LM_IDLE) { orbx_set_error("%s: %lld features do not fit a positive int32_t", fn, nfeat); return ORBX_ERR_UNSUPPORTED; }
    const int nobs = P > 0 ? t->obs_off[P] : 0, ncov = map->cov_off[K], nchild = map->child_off[K];
    // the snapshot: keyframes | points | obs_off | observations | feat_off | the features' points | parent | cov_off | cov | child_off | child | views | desc
    StagePlan pl;
    const size_t oKf = pl.take((size_t)K * sizeof(orbc_keyframe_t)), oPt = pl.take((size_t)P * sizeof(orbc_point_t)), oOff = pl.take((size_t)(P + 1) * 4),
                 oObs = pl.take((size_t)nobs * sizeof(orbc_observation_t)), oFo = pl.take((size_t)(K + 1) * 4), oFp = pl.take((size_t)nfeat * 4),
                 oPa = pl.take((size_t)K * 4), oCo = pl.take((size_t)(K + 1) * 4), oCv = pl.take((size_t)ncov * 4), oHo = pl.take((size_t)(K + 1) * 4),
                 oCh = pl.take((size_t)nchild * 4), oVw = pl.take((size_t)P * sizeof(orbt_pointview_t)), oDs = pl.take((size_t)P * 32);
    h->K = K; h->P = P; h->F = nfeat; h->snapBytes = pl.off; h->hasShape = true; h->resident = false;
    rc = lm_map_reserve(h, pl.off, (size_t)P);
    if (rc) { h->mapStatus = rc; return rc; }
    uint8_t *d = h->d_map, *m = h->h_map;
    if (K > 0) memcpy(m + oKf, t->kf, (size_t)K * sizeof(orbc_keyframe_t));
    if (P > 0) { memcpy(m + oPt, t->pts, (size_t)P * sizeof(orbc_point_t)); memcpy(m + oOff, t->obs_off, (size_t)(P + 1) * 4); }
    else memset(m + oOff, 0, 4);
    if (nobs > 0) memcpy(m + oObs, t->obs, (size_t)nobs * sizeof(orbc_observation_t));
    if (K > 0) memcpy(m + oFo, q->feat_off, (size_t)(K + 1) * 4);
    else memset(m + oFo, 0, 4);
    int32_t *fpt = (int32_t *)(m + oFp);
    for (long long f = 0; f < nfeat; f++) fpt[f] = q->feat[f].point;
    if (K > 0) memcpy(m + oPa, map->parent, (size_t)K * 4);
    memcpy(m + oCo, map->cov_off, (size_t)(K + 1) * 4);
    if (ncov > 0) memcpy(m + oCv, map->cov, (size_t)ncov * 4);
    memcpy(m + oHo, map->child_off, (size_t)(K + 1) * 4);
    if (nchild > 0) memcpy(m + oCh, map->child, (size_t)nchild * 4);
    if (P > 0) { memcpy(m + oVw, map->views, (size_t)P * sizeof(orbt_pointview_t)); memcpy(m + oDs, map->desc, (size_t)P * 32); }
    rc = lm_map_upload(h, pl.off);
    if (rc) { h->mapStatus = rc; return rc; }
    LmMap &M = h->M;
    M.T.kf = (const orbc_keyframe_t *)(d + oKf); M.T.pts = (const orbc_point_t *)(d + oPt); M.T.obs_off = (const int32_t *)(d + oOff);
    M.T.obs = (const orbc_observation_t *)(d + oObs); M.T.sf = nullptr; M.T.K = K; M.T.P = P; M.T.nlevels = t->nlevels;
    M.feat_off = (const int32_t *)(d + oFo); M.feat_pt = (const int32_t *)(d + oFp); M.parent = (const int32_t *)(d + oPa);
    M.cov_off = (const int32_t *)(d + oCo); M.cov = (const int32_t *)(d + oCv); M.child_off = (const int32_t *)(d + oHo); M.child = (const int32_t *)(d + oCh);
    M.views = (const orbt_pointview_t *)(d + oVw); M.desc = d + oDs;
    h->resident = true; h->mapStatus = ORBX_OK;
    return ORBX_OK;
}

extern "C" int orbt_update_local_map(orbt_localmap_t *h, const int32_t *frame_points, int N, const int32_t *prev_kf, int n_prev, int max_keyframes,
                                     int nbest, orbt_local_t *out) {
    const char *fn = "orbt_update_local_map";
    if (!h || !out) { orbx_set_error("%s: NULL handle or result", fn); return ORBX_ERR_ARG; }
    if (!h->hasShape) { orbx_set_error("%s: no map: call orbt_localmap_set_map first", fn); return ORBX_ERR_ARG; }
    const int K = h->K, P = h->P;
    if (N < 0 || n_prev < 0 || max_keyframes < 0 || nbest < 0 || (N > 0 && !frame_points) || (n_prev > 0 && !prev_kf)) {
        orbx_set_error("%s: bad arguments (N %d, n_prev %d, max_keyframes %d, nbest %d)", fn, N, n_prev, max_keyframes, nbest);
        return ORBX_ERR_ARG;
    }
    if ((N > 0 && (!out->frame_points || !out->holder || !out->ext_obs)) || (K > 0 && !out->local_kf) || (P > 0 && (!out->local_pts || !out->pts || !out->mp_desc))) {
        orbx_set_error("%s: bad result arrays", fn);
        return ORBX_ERR_ARG;
    }
    for (int i = 0; i < N; i++)
        if (frame_points[i] < -1 || frame_points[i] >= P) return lm_fail(fn, "frame point out of range", i, frame_points[i]);
    if (n_prev > 0) {
        std::vector<uint8_t> seen((size_t)K, 0);
        for (int j = 0; j < n_prev; j++) {
            if (prev_kf[j] < 0 || prev_kf[j] >= K) return lm_fail(fn, "prev_kf out of range", j, prev_kf[j]);
            if (seen[prev_kf[j]]) return lm_fail(fn, "prev_kf repeated", j, prev_kf[j]);
            seen[prev_kf[j]] = 1;
        }
    }
    if (!h->resident) {
        orbx_set_error("%s: the last orbt_localmap_set_map did not reach the device (status %d)", fn, h->mapStatus);
        return h->mapStatus ? h->mapStatus : ORBX_ERR_ARG;
    }
    const size_t tilesMax = (size_t)((h->F + LM_THREADS - 1) / LM_THREADS);
    // upload: the frame's points as feature records | prev_kf; download: head | fp | holder | ext_obs, then the used prefixes of
    // local_kf | local_pts | pts | mp_desc; device only: counters | kf_start | rank | tile_cnt
    StagePlan pl;
    const size_t oFe = pl.take((size_t)N * sizeof(orbc_feature_t)), oPv = pl.take((size_t)n_prev * 4);
    pl.mark_inputs();
    const size_t oHead = pl.take(sizeof(LmHead)), oFpo = pl.take((size_t)N * 4), oHol = pl.take((size_t)N * 4), oExt = pl.take((size_t)N * 4),
                 oLk = pl.take((size_t)K * 4), oLp = pl.take((size_t)P * 4), oPts = pl.take((size_t)P * sizeof(orbm_worldpoint_t)), oDs = pl.take((size_t)P * 32);
    const size_t outEnd = pl.off;
    const size_t oCnt = pl.take((size_t)K * 4), oKs = pl.take((size_t)(K + 1) * 4), oRank = pl.take((size_t)h->F * 4), oTc = pl.take(tilesMax * 4);
    int rc = lm_device(h);
    if (!rc) rc = lm_reserve(h, &h->d_frame, &h->frameCap, pl.off, &h->h_frame, &h->frameHostCap, outEnd);
    if (!rc) rc = lm_state_reserve(h, (size_t)P);
    if (rc) return rc;
    uint8_t *d = h->d_frame, *m = h->h_frame;
    const hipStream_t st = h->stream;
    orbc_feature_t *fe = (orbc_feature_t *)(m + oFe);
    for (int i = 0; i < N; i++) { fe[i].point = frame_points[i]; fe[i].octave = 0; fe[i].depth = 0.f; }
    if (n_prev > 0) memcpy(m + oPv, prev_kf, (size_t)n_prev * 4);
    LmFrame F;
    F.feat = (const orbc_feature_t *)(d + oFe); F.prev_kf = (const int32_t *)(d + oPv); F.N = N; F.n_prev = n_prev; F.max_keyframes = max_keyframes; F.nbest = nbest;
    F.counters = (int32_t *)(d + oCnt); F.first = (int32_t *)h->d_state; F.inframe = h->d_state + h->stateCap * 4; F.kf_start = (int32_t *)(d + oKs);
    F.rank = (int32_t *)(d + oRank); F.tile_cnt = (int32_t *)(d + oTc); F.head = (LmHead *)(d + oHead); F.fp = (int32_t *)(d + oFpo);
    F.holder = (int32_t *)(d + oHol); F.ext_obs = (int32_t *)(d + oExt); F.local_kf = (int32_t *)(d + oLk); F.local_pts = (int32_t *)(d + oLp);
    F.pts = (orbm_worldpoint_t *)(d + oPts); F.mp_desc = d + oDs;
    const LmMap &M = h->M;
    h->dirty = true;
    if (pl.in_end > 0) ORBX_HIP(hipMemcpyAsync(d, m, pl.in_end, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    if (K > ORBC_LDS_KEYFRAMES) ORBX_HIP(hipMemsetAsync(d + oCnt, 0, (size_t)K * 4, st));   // the global counter row: fresh scratch is not zero
    hipLaunchKernelGGL(k_lm_vote, dim3(1), dim3(COV_COUNT_THREADS), 0, st, M, F);
    hipLaunchKernelGGL(k_lm_keyframes, dim3(1), dim3(LM_KF_THREADS), 0, st, M, F);
    hipLaunchKernelGGL(k_lm_first, dim3(LM_GRID), dim3(LM_THREADS), 0, st, M, F);
    hipLaunchKernelGGL(k_lm_count, dim3(LM_GRID), dim3(LM_THREADS), 0, st, M, F);
    hipLaunchKernelGGL(k_lm_scan, dim3(1), dim3(LM_THREADS), 0, st, F);
    hipLaunchKernelGGL(k_lm_emit, dim3(LM_GRID), dim3(LM_THREADS), 0, st, M, F);
    hipLaunchKernelGGL(k_lm_holder, dim3(LM_GRID), dim3(LM_THREADS), 0, st, M, F);
    hipLaunchKernelGGL(k_lm_clean, dim3(LM_GRID), dim3(LM_THREADS), 0, st, M, F);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(m + oHead, d + oHead, oLk - oHead, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    h->dirty = false;   // the cleaning pass ran
    int syncs = 1;
    const LmHead hd = *(const LmHead *)(m + oHead);
    if (hd.n_local_kf < 0 || hd.n_local_kf > K || hd.n_local_pts < 0 || hd.n_local_pts > P) {
        orbx_set_error("%s: the device returned lengths out of range (%d keyframes, %d points)", fn, hd.n_local_kf, hd.n_local_pts);
        return ORBX_ERR_HIP;
    }
    const size_t nk = (size_t)hd.n_local_kf, np = (size_t)hd.n_local_pts;
    if (nk > 0) ORBX_HIP(hipMemcpyAsync(m + oLk, d + oLk, nk * 4, hipMemcpyDeviceToHost, st));
    if (np > 0) {
        ORBX_HIP(hipMemcpyAsync(m + oLp, d + oLp, np * 4, hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipMemcpyAsync(m + oPts, d + oPts, np * sizeof(orbm_worldpoint_t), hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipMemcpyAsync(m + oDs, d + oDs, np * 32, hipMemcpyDeviceToHost, st));
    }
    if (nk > 0 || np > 0) { ORBX_HIP(hipStreamSynchronize(st)); syncs = 2; }
    if (N > 0) { memcpy(out->frame_points, m + oFpo, (size_t)N * 4); memcpy(out->holder, m + oHol, (size_t)N * 4); memcpy(out->ext_obs, m + oExt, (size_t)N * 4); }
    if (nk > 0) memcpy(out->local_kf, m + oLk, nk * 4);
    if (np > 0) { memcpy(out->local_pts, m + oLp, np * 4); memcpy(out->pts, m + oPts, np * sizeof(orbm_worldpoint_t)); memcpy(out->mp_desc, m + oDs, np * 32); }
    out->n_local_kf = hd.n_local_kf; out->n_local_pts = hd.n_local_pts;
    orbt_local_info_t &info = out->info;
    info.empty_vote = hd.empty_vote; info.n_voted = hd.n_voted; info.ref_kf = hd.ref_kf; info.ref_votes = hd.ref_votes; info.extension_end = hd.extension_end;
    info.launches = 8; info.syncs = syncs; info.pad = 0;
    return ORBX_OK;
}
