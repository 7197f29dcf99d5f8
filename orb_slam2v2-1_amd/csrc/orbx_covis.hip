// orbx_covis.hip — covisibility on the device (row a33, prefix orbc_): KeyFrame::UpdateConnections (reference: src/KeyFrame.cc:290-380),
// LocalMapping::KeyFrameCulling (src/LocalMapping.cc:640-704) and MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:340-383) over one
// observation table (include/orbx.h).  The kernels' bodies are in orbx_covis_dev.h, which tests/cpp/covis_lockstep.cc compiles for
// the host; here are the kernels around them, the radix path of k_cov_order for lists longer than ORBC_SORT_LDS (the shared core of
// orbx_cloud_dev.h) and the host side: the checks, the packing of the staging block and the launches.  DESIGN.md section 6, "k_cov_*".
#include "orbx_stage.h"
#include "orbx_cloud_dev.h"
#include "orbx_covis_dev.h"

static_assert(COV_ORDER_THREADS == CL_THREADS, "k_cov_order runs the radix core's workgroup");
static_assert(sizeof(orbc_keyframe_t) == 24 && sizeof(orbc_point_t) == 20 && sizeof(orbc_observation_t) == 12 && sizeof(orbc_feature_t) == 12 &&
              sizeof(orbc_normal_t) == 24, "record sizes of include/orbx.h");

// One workgroup per query.  K <= ORBC_LDS_KEYFRAMES: the counters live in LDS and every entry of the query's row is stored at the end
// (nobody zeroed the row).  Beyond: the adds go to the row itself, which the call zeroed in its own stream.
__global__ __launch_bounds__(COV_COUNT_THREADS) void k_cov_count(CovTable T, CovQueries Qs, int32_t *counters) {
    __shared__ int32_t tab[ORBC_LDS_KEYFRAMES];
    const int q = blockIdx.x, s = Qs.query_kf[q];
    int32_t *row = counters + (size_t)q * T.K;
    const bool lds = T.K <= ORBC_LDS_KEYFRAMES;
    if (lds) {
        for (int k = threadIdx.x; k < T.K; k += COV_COUNT_THREADS) tab[k] = 0;
        __syncthreads();
    }
    cov_count_query(T, Qs.feat, Qs.feat_off[q], Qs.feat_off[q + 1], s, lds ? tab : row);
    if (lds) {
        __syncthreads();
        for (int k = threadIdx.x; k < T.K; k += COV_COUNT_THREADS) row[k] = tab[k];
    }
}

// keys[0..n) of one query, ascending, by the LSD radix core: npass passes of 8 bits between a and b; hist: [tiles][256] words.
// Returns the buffer that holds the result.  One workgroup walks its tiles one after the other: a pass is the three launches of
// orbx_cloud.hip (histogram, scan, scatter) as three loops
__device__ const unsigned long long *cov_sort_radix(unsigned long long *a, unsigned long long *b, int n, int npass, uint32_t *hist,
                                                    uint32_t *sh, uint32_t (*seg)[256], int *scanLds) {
    const int tiles = (n + CL_TILE - 1) / CL_TILE;
    unsigned long long *src = a, *dst = b;
    for (int pass = 0; pass < npass; pass++) {
        for (int t = 0; t < tiles; t++) {
            radix_tile_hist(src, n, t * CL_TILE, pass, sh);
            hist[t * 256 + threadIdx.x] = sh[threadIdx.x];   // lane d owns column d of hist: only it reads the column below
            __syncthreads();
        }
        uint32_t tot = 0;
        for (int t = 0; t < tiles; t++) tot += hist[t * 256 + threadIdx.x];
        int total;
        uint32_t run = (uint32_t)block_excl_scan((int)tot, scanLds, total);
        for (int t = 0; t < tiles; t++) { const uint32_t c = hist[t * 256 + threadIdx.x]; hist[t * 256 + threadIdx.x] = run; run += c; }
        for (int t = 0; t < tiles; t++) {
            unsigned long long key[CL_ITERS];
            bool flag[CL_ITERS];
#pragma unroll
            for (int k = 0; k < CL_ITERS; k++) {
                const int i = tile_elem(t * CL_TILE, k);
                flag[k] = i < n;
                key[k] = flag[k] ? src[i] : 0ull;
            }
            for (int sgm = 0; sgm < CL_SEGS; sgm++) seg[sgm][threadIdx.x] = 0u;
            __syncthreads();
            radix_tile_scatter(key, flag, pass, n, seg, [&]() { return hist[t * 256 + threadIdx.x]; }, [&](int k, uint32_t o) { dst[o] = key[k]; });
            __syncthreads();
        }
        unsigned long long *x = src; src = dst; dst = x;
    }
    return src;
}

// One workgroup per query.  keys: [Q][2][K] words and hist: [Q][tiles(K)][256], both NULL when K <= ORBC_SORT_LDS (no list can be longer)
__global__ __launch_bounds__(COV_ORDER_THREADS) void k_cov_order(const int32_t *counters, int K, int th, int cap, int sb, int32_t *ids, int32_t *weights,
                                                                  int32_t *nOut, unsigned long long *keys, uint32_t *hist) {
    __shared__ unsigned long long sKeys[ORBC_SORT_LDS];
    __shared__ unsigned long long sBest;
    __shared__ int sCnt, sWave[COV_ORDER_THREADS / COV_WAVE], scanLds[4];
    __shared__ uint32_t sh[256], seg[CL_SEGS][256];
    const int q = blockIdx.x;
    const int32_t *row = counters + (size_t)q * K;
    ids += (size_t)q * cap; weights += (size_t)q * cap;
    cov_order_scan(row, K, th, &sCnt, &sBest);
    const int n = sCnt;
    if (n == 0) { cov_order_single(sBest, cap, ids, weights, nOut + q); return; }
    if (threadIdx.x == 0) nOut[q] = n;
    if (n <= ORBC_SORT_LDS) {
        cov_order_compact(row, K, th, sb, sKeys, sWave);
        cov_sort_lds(sKeys, n);
        cov_order_emit(sKeys, n, 0, sb, cap, ids, weights);
        return;
    }
    unsigned long long *a = keys + (size_t)q * 2 * K, *b = a + K;
    cov_order_compact(row, K, th, sb, a, sWave);
    int wbits = 0;
    for (unsigned long long w = sBest >> 32; w; w >>= 1) wbits++;   // the largest weight
    const int tilesK = (K + CL_TILE - 1) / CL_TILE;
    const unsigned long long *res = cov_sort_radix(a, b, n, (sb + wbits + 7) / 8, hist + (size_t)q * tilesK * 256, sh, seg, scanLds);
    cov_order_emit(res, n, 1, sb, cap, ids, weights);
}

__global__ __launch_bounds__(COV_CULL_THREADS) void k_cull(CovTable T, CovQueries Qs, int monocular, int th_obs, int32_t *n_mps, int32_t *n_red,
                                                            int32_t *verdict, uint8_t *point_bad) {
    __shared__ uint32_t bits[ORBC_MAX_CULL_KEYFRAMES / 32];
    __shared__ int sM, sR;
    cov_cull(T, Qs, monocular, th_obs, n_mps, n_red, verdict, point_bad, bits, &sM, &sR);
}

// One thread per point; Ow is gathered from the K-entry keyframe array
__global__ __launch_bounds__(COV_NORMAL_THREADS) void k_normals(CovTable T, orbc_normal_t *out) {
    const int p = blockIdx.x * COV_NORMAL_THREADS + threadIdx.x;
    if (p < T.P) out[p] = cov_normal(T, p);
}

// ---------------------------------------------------------------- host side
static thread_local StagePair g_cv;
void orbx_internal_release_covis_scratch() { g_cv.release(); }

static int cov_fail(const char *fn, const char *what, long long at, long long v) {
    orbx_set_error("%s: %s (at %lld: %lld)", fn, what, at, v);
    return ORBX_ERR_ARG;
}

// the table's own ranges
static int cov_check_table(const char *fn, const orbc_table_t *t) {
    if (!t || t->K < 0 || t->P < 0 || (t->K > 0 && !t->kf) || (t->P > 0 && (!t->pts || !t->obs_off)) || t->nlevels < 1 || !t->scale_factors) {
        orbx_set_error("%s: bad table arguments", fn);
        return ORBX_ERR_ARG;
    }
    if (t->P == 0) return ORBX_OK;
    if (t->obs_off[0] != 0) return cov_fail(fn, "obs_off does not start at 0", 0, t->obs_off[0]);
    for (int p = 0; p < t->P; p++) {
        const int lo = t->obs_off[p], hi = t->obs_off[p + 1];
        if (hi < lo) return cov_fail(fn, "obs_off decreases", p + 1, hi);
        if (hi > lo && !t->obs) { orbx_set_error("%s: bad table arguments", fn); return ORBX_ERR_ARG; }
        if (t->pts[p].ref_kf < -1 || t->pts[p].ref_kf >= t->K) return cov_fail(fn, "ref_kf out of range", p, t->pts[p].ref_kf);
        for (int o = lo; o < hi; o++) {
            const orbc_observation_t &ob = t->obs[o];
            if (ob.kf < 0 || ob.kf >= t->K) return cov_fail(fn, "observation kf out of range", o, ob.kf);
            if (o > lo && ob.kf <= t->obs[o - 1].kf) return cov_fail(fn, "observation kf not strictly ascending in a point's list", o, ob.kf);
            if (ob.idx < 0) return cov_fail(fn, "observation idx negative", o, ob.idx);
            if (ob.octave >= t->nlevels) return cov_fail(fn, "observation octave out of range", o, ob.octave);
        }
    }
    return ORBX_OK;
}

static int cov_check_queries(const char *fn, const orbc_table_t *t, const orbc_queries_t *q, bool distinct) {
    if (!q || q->Q < 0 || (q->Q > 0 && (!q->query_kf || !q->feat_off))) { orbx_set_error("%s: bad query arguments", fn); return ORBX_ERR_ARG; }
    if (q->Q == 0) return ORBX_OK;
    if (q->feat_off[0] != 0) return cov_fail(fn, "feat_off does not start at 0", 0, q->feat_off[0]);
    std::vector<uint8_t> seen(distinct ? (size_t)t->K : 0, 0);
    for (int i = 0; i < q->Q; i++) {
        const int s = q->query_kf[i], lo = q->feat_off[i], hi = q->feat_off[i + 1];
        if (s < 0 || s >= t->K) return cov_fail(fn, "query_kf out of range", i, s);
        if (distinct) { if (seen[s]) return cov_fail(fn, "query keyframe repeated", i, s); seen[s] = 1; }
        if (hi < lo) return cov_fail(fn, "feat_off decreases", i + 1, hi);
        if (hi > lo && !q->feat) { orbx_set_error("%s: bad query arguments", fn); return ORBX_ERR_ARG; }
        for (int f = lo; f < hi; f++) {
            if (q->feat[f].point < -1 || q->feat[f].point >= t->P) return cov_fail(fn, "feature point out of range", f, q->feat[f].point);
            if (q->feat[f].octave < 0 || q->feat[f].octave >= t->nlevels) return cov_fail(fn, "feature octave out of range", f, q->feat[f].octave);
        }
    }
    return ORBX_OK;
}

struct CovQOff { size_t kf, off, feat; };
static CovQOff cov_take_queries(StagePlan &pl, const orbc_queries_t *q) {
    CovQOff o;
    o.kf = pl.take((size_t)q->Q * 4); o.off = pl.take((size_t)(q->Q + 1) * 4); o.feat = pl.take((size_t)(q->Q > 0 ? q->feat_off[q->Q] : 0) * sizeof(orbc_feature_t));
    return o;
}
static CovQueries cov_put_queries(uint8_t *h, uint8_t *d, const CovQOff &o, const orbc_queries_t *q) {
    if (q->Q > 0) {
        memcpy(h + o.kf, q->query_kf, (size_t)q->Q * 4);
        memcpy(h + o.off, q->feat_off, (size_t)(q->Q + 1) * 4);
        if (q->feat_off[q->Q] > 0) memcpy(h + o.feat, q->feat, (size_t)q->feat_off[q->Q] * sizeof(orbc_feature_t));
    } else memset(h + o.off, 0, 4);
    CovQueries r;
    r.query_kf = (const int32_t *)(d + o.kf); r.feat_off = (const int32_t *)(d + o.off); r.feat = (const orbc_feature_t *)(d + o.feat); r.Q = q->Q;
    return r;
}

extern "C" int orbc_covisibility(const orbc_table_t *table, const orbc_queries_t *conn_queries, const orbc_connections_t *conn,
                                 const orbc_queries_t *cull_queries, const orbc_culling_t *cull, orbc_normal_t *normals, int device) {
    const char *fn = "orbc_covisibility";
    int rc = cov_check_table(fn, table);
    if (rc) return rc;
    const int K = table->K, P = table->P;
    int Qc = 0, Qk = 0;
    if (conn) {
        rc = cov_check_queries(fn, table, conn_queries, false);
        if (rc) return rc;
        Qc = conn_queries->Q;
        if (conn->th < 1) return cov_fail(fn, "th below 1", 0, conn->th);
        if (conn->cap < 0) return cov_fail(fn, "cap negative", 0, conn->cap);
        if (Qc > 0 && (!conn->n || (conn->cap > 0 && (!conn->ids || !conn->weights)))) { orbx_set_error("%s: bad connection outputs", fn); return ORBX_ERR_ARG; }
    }
    if (cull) {
        rc = cov_check_queries(fn, table, cull_queries, true);
        if (rc) return rc;
        Qk = cull_queries->Q;
        if (Qk > 0 && (!cull->n_mps || !cull->n_redundant || !cull->verdict)) { orbx_set_error("%s: bad culling outputs", fn); return ORBX_ERR_ARG; }
        if (K > ORBC_MAX_CULL_KEYFRAMES) { orbx_set_error("%s: %d keyframes in a culling call, at most %d", fn, K, ORBC_MAX_CULL_KEYFRAMES); return ORBX_ERR_UNSUPPORTED; }
    }
    const bool doConn = conn && Qc > 0, doCull = cull && (Qk > 0 || (cull->point_bad && P > 0)), doNorm = normals && P > 0;
    if (!doConn && !doCull && !doNorm) return ORBX_OK;
    const int nobs = P > 0 ? table->obs_off[P] : 0, cap = conn ? conn->cap : 0;
    // upload block: keyframes | points | obs_off | observations | scale factors | the two query sets;
    // download block: ids | weights | n | counters if asked for | n_mps | n_redundant | verdict | point_bad | normals; device only: the counters
    // otherwise, the radix path's keys and histograms (the pinned mirror has the pair's one size, so it grows by these too: DESIGN.md section 4a)
    StagePlan pl;
    const size_t oKf = pl.take((size_t)K * sizeof(orbc_keyframe_t)), oPt = pl.take((size_t)P * sizeof(orbc_point_t)), oOff = pl.take((size_t)(P + 1) * 4),
                 oObs = pl.take((size_t)nobs * sizeof(orbc_observation_t)), oSf = pl.take((size_t)table->nlevels * 4);
    CovQOff oqc = {0, 0, 0}, oqk = {0, 0, 0};
    if (doConn) oqc = cov_take_queries(pl, conn_queries);
    if (doCull) oqk = cov_take_queries(pl, cull_queries);
    pl.mark_inputs();
    const size_t oOut = pl.off;
    size_t oIds = 0, oW = 0, oN = 0, oCnt = 0, oM = 0, oR = 0, oV = 0, oPb = 0, oNrm = 0, oKeys = 0, oHist = 0;
    if (doConn) { oIds = pl.take((size_t)Qc * cap * 4); oW = pl.take((size_t)Qc * cap * 4); oN = pl.take((size_t)Qc * 4); if (conn->counters) oCnt = pl.take((size_t)Qc * K * 4); }
    if (doCull) { oM = pl.take((size_t)Qk * 4); oR = pl.take((size_t)Qk * 4); oV = pl.take((size_t)Qk * 4); oPb = pl.take(cull->point_bad ? (size_t)P : 0); }
    if (doNorm) oNrm = pl.take((size_t)P * sizeof(orbc_normal_t));
    const size_t oEnd = pl.off;
    const bool radix = doConn && K > ORBC_SORT_LDS;
    const int tilesK = (K + CL_TILE - 1) / CL_TILE;
    if (doConn && !conn->counters) oCnt = pl.take((size_t)Qc * K * 4);   // nobody asked for the counters: behind the downloaded block
    if (radix) { oKeys = pl.take((size_t)Qc * 2 * K * 8); oHist = pl.take((size_t)Qc * tilesK * 256 * 4); }
    rc = g_cv.reserve(device, pl.off, (size_t)1 << 18);
    if (rc) return rc;
    uint8_t *d = g_cv.d, *h = g_cv.h;
    const hipStream_t st = g_cv.stream;
    if (K > 0) memcpy(h + oKf, table->kf, (size_t)K * sizeof(orbc_keyframe_t));
    if (P > 0) { memcpy(h + oPt, table->pts, (size_t)P * sizeof(orbc_point_t)); memcpy(h + oOff, table->obs_off, (size_t)(P + 1) * 4); }
    else memset(h + oOff, 0, 4);
    if (nobs > 0) memcpy(h + oObs, table->obs, (size_t)nobs * sizeof(orbc_observation_t));
    memcpy(h + oSf, table->scale_factors, (size_t)table->nlevels * 4);
    CovTable T;
    T.kf = (const orbc_keyframe_t *)(d + oKf); T.pts = (const orbc_point_t *)(d + oPt); T.obs_off = (const int32_t *)(d + oOff);
    T.obs = (const orbc_observation_t *)(d + oObs); T.sf = (const float *)(d + oSf); T.K = K; T.P = P; T.nlevels = table->nlevels;
    CovQueries qc = {}, qk = {};
    if (doConn) qc = cov_put_queries(h, d, oqc, conn_queries);
    if (doCull) qk = cov_put_queries(h, d, oqk, cull_queries);
    ORBX_HIP(hipMemcpyAsync(d, h, pl.in_end, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    if (doConn) {
        // the global counter path adds into rows that fresh scratch does not zero; ids / weights beyond n are never read back
        if (K > ORBC_LDS_KEYFRAMES) ORBX_HIP(hipMemsetAsync(d + oCnt, 0, (size_t)Qc * K * 4, st));
        int sb = 1;
        while ((1ll << sb) < (long long)K) sb++;
        hipLaunchKernelGGL(k_cov_count, dim3(Qc), dim3(COV_COUNT_THREADS), 0, st, T, qc, (int32_t *)(d + oCnt));
        hipLaunchKernelGGL(k_cov_order, dim3(Qc), dim3(COV_ORDER_THREADS), 0, st, (const int32_t *)(d + oCnt), K, conn->th, cap, sb, (int32_t *)(d + oIds),
                           (int32_t *)(d + oW), (int32_t *)(d + oN), radix ? (unsigned long long *)(d + oKeys) : nullptr, radix ? (uint32_t *)(d + oHist) : nullptr);
    }
    if (doCull)
        hipLaunchKernelGGL(k_cull, dim3(1), dim3(COV_CULL_THREADS), 0, st, T, qk, cull->monocular, cull->th_obs, (int32_t *)(d + oM), (int32_t *)(d + oR),
                           (int32_t *)(d + oV), cull->point_bad ? d + oPb : (uint8_t *)nullptr);
    if (doNorm)
        hipLaunchKernelGGL(k_normals, dim3((P + COV_NORMAL_THREADS - 1) / COV_NORMAL_THREADS), dim3(COV_NORMAL_THREADS), 0, st, T, (orbc_normal_t *)(d + oNrm));
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(h + oOut, d + oOut, oEnd - oOut, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    if (doConn) {
        const int32_t *hn = (const int32_t *)(h + oN);
        memcpy(conn->n, hn, (size_t)Qc * 4);
        for (int q = 0; q < Qc; q++) {
            const int m = hn[q] < cap ? hn[q] : cap;
            if (m > 0) {
                memcpy(conn->ids + (size_t)q * cap, h + oIds + (size_t)q * cap * 4, (size_t)m * 4);
                memcpy(conn->weights + (size_t)q * cap, h + oW + (size_t)q * cap * 4, (size_t)m * 4);
            }
        }
        if (conn->counters) memcpy(conn->counters, h + oCnt, (size_t)Qc * K * 4);
    }
    if (doCull) {
        memcpy(cull->n_mps, h + oM, (size_t)Qk * 4); memcpy(cull->n_redundant, h + oR, (size_t)Qk * 4); memcpy(cull->verdict, h + oV, (size_t)Qk * 4);
        if (cull->point_bad) memcpy(cull->point_bad, h + oPb, (size_t)P);
    }
    if (doNorm) memcpy(normals, h + oNrm, (size_t)P * sizeof(orbc_normal_t));
    return ORBX_OK;
}

extern "C" int orbc_update_connections(const orbc_table_t *table, const orbc_queries_t *queries, int th, int cap, int32_t *ids, int32_t *weights,
                                       int32_t *n, int32_t *counters, int device) {
    if (!queries) { orbx_set_error("orbc_update_connections: bad query arguments"); return ORBX_ERR_ARG; }
    const orbc_connections_t c = {th, cap, ids, weights, n, counters};
    return orbc_covisibility(table, queries, &c, nullptr, nullptr, nullptr, device);
}

extern "C" int orbc_keyframe_culling(const orbc_table_t *table, const orbc_queries_t *queries, int monocular, int th_obs, int32_t *n_mps,
                                     int32_t *n_redundant, int32_t *verdict, uint8_t *point_bad, int device) {
    if (!queries) { orbx_set_error("orbc_keyframe_culling: bad query arguments"); return ORBX_ERR_ARG; }
    const orbc_culling_t c = {monocular, th_obs, n_mps, n_redundant, verdict, point_bad};
    return orbc_covisibility(table, nullptr, nullptr, queries, &c, nullptr, device);
}

extern "C" int orbc_update_normal_and_depth(const orbc_table_t *table, orbc_normal_t *normals, int device) {
    if (!normals && table && table->P > 0) { orbx_set_error("orbc_update_normal_and_depth: bad arguments"); return ORBX_ERR_ARG; }
    return orbc_covisibility(table, nullptr, nullptr, nullptr, nullptr, normals, device);
}

// the two checks above for the other users of the table (orbx_localmap.hip)
int orbx_internal_cov_check_table(const char *fn, const orbc_table_t *t) { return cov_check_table(fn, t); }
int orbx_internal_cov_check_queries(const char *fn, const orbc_table_t *t, const orbc_queries_t *q, bool distinct) { return cov_check_queries(fn, t, q, distinct); }
