// orbx_mapcorrect.hip — loop map correction on the device (row a36, prefix orbr_): the two map-sized loops of LoopClosing, the pose and
// point correction of CorrectLoop (reference: src/LoopClosing.cc:444-525) and the spread of a global bundle adjustment through the
// spanning tree (src/LoopClosing.cc:685-746), over the tables of include/orbx.h.  The kernels' bodies are in orbx_mapcorrect_dev.h,
// which tests/cpp/mapcorrect_lockstep.cc compiles for the host; here are the kernels around them and the host side: the checks, the
// graph work of the spread, the packing of the staging block and the launches.  DESIGN.md section 6, "k_mc_*".
#include "orbx_stage.h"
#include "orbx_mapcorrect_dev.h"
#include "orbx_mapcorrect_plan.h"

static_assert(sizeof(orbg_sim3_t) == 64 && sizeof(orbc_normal_t) == 24, "record sizes of include/orbx.h");

// One thread per query; the same grid sets every point's owner to "none" for k_mc_owner's minimum
__global__ __launch_bounds__(MC_THREADS) void k_mc_sim3(McLoop L, int32_t *owner, int P) {
    MC_FOR(q, L.Q) mc_sim3(L, q);
    MC_FOR(p, P) owner[p] = MC_NO_OWNER;
}
// One thread per feature of the queries' concatenated lists
__global__ __launch_bounds__(MC_THREADS) void k_mc_owner(CovTable T, CovQueries Qs, int nfeat, int32_t *owner) {
    MC_FOR(f, nfeat) mc_owner(T, Qs, f, owner);
}
// One thread per point
__global__ __launch_bounds__(MC_THREADS) void k_mc_points(CovTable T, McPoints M) {
    MC_FOR(p, T.P) mc_point(T, M, p);
}
// One thread per keyframe of one level: order[first .. first + n)
__global__ __launch_bounds__(MC_THREADS) void k_mc_tree(McTree G, int first, int n) {
    MC_FOR(i, n) mc_tree(G, G.order[first + i]);
}
// One thread per point
__global__ __launch_bounds__(MC_THREADS) void k_mc_spread(McSpread S, int P) {
    MC_FOR(p, P) mc_spread(S, p);
}

// ---------------------------------------------------------------- host side
static thread_local StagePair g_mc;
void orbx_internal_release_mapcorrect_scratch() { g_mc.release(); }

static int mc_fail(const char *fn, const char *what, long long at, long long v) {
    orbx_set_error("%s: %s (at %lld: %lld)", fn, what, at, v);
    return ORBX_ERR_ARG;
}
static inline int mc_blocks(int n) { return n > 0 ? (n + MC_THREADS - 1) / MC_THREADS : 1; }

extern "C" int orbr_correct_loop(const orbc_table_t *table, const orbc_queries_t *conn, int32_t cur, const float *Tiw16, const orbg_sim3_t *Scw,
                                 const orbr_loop_out_t *out, int device) {
    const char *fn = "orbr_correct_loop";
    int rc = orbx_internal_cov_check_table(fn, table);
    if (rc) return rc;
    rc = orbx_internal_cov_check_queries(fn, table, conn, false);
    if (rc) return rc;
    if (!Tiw16 || !Scw || !out || !out->corrected || !out->non_corrected || !out->Tiw_new16 || !out->Ow_new3 || !out->corrected_ref || !out->normals ||
        (table->P > 0 && !out->pos3)) {
        orbx_set_error("%s: bad arguments", fn);
        return ORBX_ERR_ARG;
    }
    const int K = table->K, P = table->P, Q = conn->Q;
    if (cur < 0 || cur >= K) return mc_fail(fn, "cur out of range", 0, cur);
    int curPos = -1;
    for (int q = 0; q < Q; q++) {
        if (q > 0 && conn->query_kf[q] <= conn->query_kf[q - 1]) return mc_fail(fn, "query_kf not strictly ascending", q, conn->query_kf[q]);
        if (conn->query_kf[q] == cur) curPos = q;
    }
    if (curPos < 0) return mc_fail(fn, "cur is not among the queries", 0, cur);
    const int nobs = P > 0 ? table->obs_off[P] : 0, nfeat = conn->feat_off[Q];
    // upload block: keyframes | points | obs_off | observations | scale factors | query_kf | feat_off | features | qpos | Tiw;
    // download block: corrected | non_corrected | Tiw_new | Ow_new | pos | corrected_ref | normals; device only: corrected^-1 | owner
    StagePlan pl;
    const size_t oKf = pl.take((size_t)K * sizeof(orbc_keyframe_t)), oPt = pl.take((size_t)P * sizeof(orbc_point_t)), oOff = pl.take((size_t)(P + 1) * 4),
                 oObs = pl.take((size_t)nobs * sizeof(orbc_observation_t)), oSf = pl.take((size_t)table->nlevels * 4), oQk = pl.take((size_t)Q * 4),
                 oFo = pl.take((size_t)(Q + 1) * 4), oFt = pl.take((size_t)nfeat * sizeof(orbc_feature_t)), oQp = pl.take((size_t)K * 4),
                 oTiw = pl.take((size_t)Q * 64);
    pl.mark_inputs();
    const size_t oOut = pl.off;
    const size_t oC = pl.take((size_t)Q * sizeof(orbg_sim3_t)), oN = pl.take((size_t)Q * sizeof(orbg_sim3_t)), oTn = pl.take((size_t)Q * 64),
                 oOw = pl.take((size_t)Q * 12), oPos = pl.take((size_t)P * 12), oRef = pl.take((size_t)P * 4), oNrm = pl.take((size_t)P * sizeof(orbc_normal_t));
    const size_t oEnd = pl.off;
    const size_t oCi = pl.take((size_t)Q * sizeof(orbg_sim3_t)), oOwn = pl.take((size_t)P * 4);
    rc = g_mc.reserve(device, pl.off, (size_t)1 << 18);
    if (rc) return rc;
    uint8_t *d = g_mc.d, *h = g_mc.h;
    const hipStream_t st = g_mc.stream;
    memcpy(h + oKf, table->kf, (size_t)K * sizeof(orbc_keyframe_t));
    if (P > 0) { memcpy(h + oPt, table->pts, (size_t)P * sizeof(orbc_point_t)); memcpy(h + oOff, table->obs_off, (size_t)(P + 1) * 4); }
    else memset(h + oOff, 0, 4);
    if (nobs > 0) memcpy(h + oObs, table->obs, (size_t)nobs * sizeof(orbc_observation_t));
    memcpy(h + oSf, table->scale_factors, (size_t)table->nlevels * 4);
    memcpy(h + oQk, conn->query_kf, (size_t)Q * 4);
    memcpy(h + oFo, conn->feat_off, (size_t)(Q + 1) * 4);
    if (nfeat > 0) memcpy(h + oFt, conn->feat, (size_t)nfeat * sizeof(orbc_feature_t));
    int32_t *qpos = (int32_t *)(h + oQp);   // slot -> position among the queries, -1 for a keyframe that is not one
    for (int k = 0; k < K; k++) qpos[k] = -1;
    for (int q = 0; q < Q; q++) qpos[conn->query_kf[q]] = q;
    memcpy(h + oTiw, Tiw16, (size_t)Q * 64);
    CovTable T;
    T.kf = (const orbc_keyframe_t *)(d + oKf); T.pts = (const orbc_point_t *)(d + oPt); T.obs_off = (const int32_t *)(d + oOff);
    T.obs = (const orbc_observation_t *)(d + oObs); T.sf = (const float *)(d + oSf); T.K = K; T.P = P; T.nlevels = table->nlevels;
    CovQueries Qs;
    Qs.query_kf = (const int32_t *)(d + oQk); Qs.feat_off = (const int32_t *)(d + oFo); Qs.feat = (const orbc_feature_t *)(d + oFt); Qs.Q = Q;
    McLoop L;
    L.Tiw = (const float *)(d + oTiw); L.Scw = *Scw; L.Q = Q; L.cur_pos = curPos; L.corrected = (orbg_sim3_t *)(d + oC); L.non_corrected = (orbg_sim3_t *)(d + oN);
    L.corrected_inv = (orbg_sim3_t *)(d + oCi); L.Tiw_new = (float *)(d + oTn); L.Ow_new = (float *)(d + oOw);
    McPoints M;
    M.qpos = (const int32_t *)(d + oQp); M.query_kf = Qs.query_kf; M.owner = (const int32_t *)(d + oOwn); M.non_corrected = L.non_corrected;
    M.corrected_inv = L.corrected_inv; M.Ow_new = L.Ow_new; M.pos = (float *)(d + oPos); M.corrected_ref = (int32_t *)(d + oRef);
    M.normals = (orbc_normal_t *)(d + oNrm);
    ORBX_HIP(hipMemcpyAsync(d, h, pl.in_end, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_mc_sim3, dim3(mc_blocks(Q > P ? Q : P)), dim3(MC_THREADS), 0, st, L, (int32_t *)(d + oOwn), P);
    hipLaunchKernelGGL(k_mc_owner, dim3(mc_blocks(nfeat)), dim3(MC_THREADS), 0, st, T, Qs, nfeat, (int32_t *)(d + oOwn));
    hipLaunchKernelGGL(k_mc_points, dim3(mc_blocks(P)), dim3(MC_THREADS), 0, st, T, M);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(h + oOut, d + oOut, oEnd - oOut, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    memcpy(out->corrected, h + oC, (size_t)Q * sizeof(orbg_sim3_t));
    memcpy(out->non_corrected, h + oN, (size_t)Q * sizeof(orbg_sim3_t));
    memcpy(out->Tiw_new16, h + oTn, (size_t)Q * 64);
    memcpy(out->Ow_new3, h + oOw, (size_t)Q * 12);
    if (P > 0) {
        memcpy(out->pos3, h + oPos, (size_t)P * 12);
        memcpy(out->corrected_ref, h + oRef, (size_t)P * 4);
        memcpy(out->normals, h + oNrm, (size_t)P * sizeof(orbc_normal_t));
    }
    return ORBX_OK;
}

extern "C" int orbr_spread_global_ba(const orbr_spread_in_t *in, orbr_spread_out_t *out, int device) {
    const char *fn = "orbr_spread_global_ba";
    if (!in || !out || in->K < 0 || in->P < 0 || in->n_origins < 0 || !in->child_off || (in->n_origins > 0 && !in->origins) ||
        (in->K > 0 && (!in->Tcw16 || !in->TcwGBA16 || !in->kf_in_gba || !out->Tcw_new16 || !out->TcwGBA_out16 || !out->kf_marked)) ||
        (in->P > 0 && (!in->pos3 || !in->posGBA3 || !in->pt_in_gba || !in->ref_kf || !in->bad || !out->pos_out3 || !out->status))) {
        orbx_set_error("%s: bad arguments", fn);
        return ORBX_ERR_ARG;
    }
    const int K = in->K, P = in->P;
    out->levels = 0;
    // the graph work (orbx_mapcorrect_plan.h): parents from the child lists, the walk of :686-709 as a breadth-first pass, the levels
    McSpreadPlan gp;
    if (!mc_plan_spread(in, gp)) return mc_fail(fn, gp.what, gp.at, gp.v);
    const std::vector<int32_t> &parent = gp.parent, &order = gp.order, &first = gp.first;
    const std::vector<uint8_t> &reached = gp.reached, &marked = gp.marked;
    const int nlev = gp.levels;
    out->levels = nlev;
    if (K == 0 && P == 0) return ORBX_OK;
    const int norder = (int)order.size();
    // upload block: Tcw | TcwGBA | parent | order | reached | marked | pos | posGBA | pt_in_gba | bad | ref_kf; download block: TcwGBA | pos_out | status.
    // TcwGBA is uploaded into the download block: the levels write it in place
    StagePlan pl;
    const size_t oTcw = pl.take((size_t)K * 64), oPar = pl.take((size_t)K * 4), oOrd = pl.take((size_t)norder * 4), oRea = pl.take((size_t)K), oMar = pl.take((size_t)K),
                 oPos = pl.take((size_t)P * 12), oPg = pl.take((size_t)P * 12), oIn = pl.take((size_t)P), oBad = pl.take((size_t)P), oRef = pl.take((size_t)P * 4),
                 oGba = pl.take((size_t)K * 64);
    pl.mark_inputs();
    const size_t oOut = oGba;
    const size_t oPo = pl.take((size_t)P * 12), oSt = pl.take((size_t)P * 4);
    const int rc = g_mc.reserve(device, pl.off, (size_t)1 << 18);
    if (rc) return rc;
    uint8_t *d = g_mc.d, *h = g_mc.h;
    const hipStream_t st = g_mc.stream;
    if (K > 0) {
        memcpy(h + oTcw, in->Tcw16, (size_t)K * 64);
        memcpy(h + oGba, in->TcwGBA16, (size_t)K * 64);
        memcpy(h + oPar, parent.data(), (size_t)K * 4);
        memcpy(h + oRea, reached.data(), (size_t)K);
        memcpy(h + oMar, marked.data(), (size_t)K);
    }
    if (norder > 0) memcpy(h + oOrd, order.data(), (size_t)norder * 4);
    if (P > 0) {
        memcpy(h + oPos, in->pos3, (size_t)P * 12); memcpy(h + oPg, in->posGBA3, (size_t)P * 12); memcpy(h + oIn, in->pt_in_gba, (size_t)P);
        memcpy(h + oBad, in->bad, (size_t)P); memcpy(h + oRef, in->ref_kf, (size_t)P * 4);
    }
    McTree G;
    G.Tcw = (const float *)(d + oTcw); G.TcwGBA = (float *)(d + oGba); G.parent = (const int32_t *)(d + oPar); G.order = (const int32_t *)(d + oOrd);
    McSpread S;
    S.Tcw = G.Tcw; S.TcwGBA = G.TcwGBA; S.pos = (const float *)(d + oPos); S.posGBA = (const float *)(d + oPg); S.pt_in_gba = d + oIn; S.bad = d + oBad;
    S.reached = d + oRea; S.marked = d + oMar; S.ref_kf = (const int32_t *)(d + oRef); S.pos_out = (float *)(d + oPo); S.status = (int32_t *)(d + oSt);
    ORBX_HIP(hipMemcpyAsync(d, h, pl.in_end, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    for (int l = 1; l <= nlev; l++)   // a level's parents are of the level below, or inside the global BA: final when this launch starts
        hipLaunchKernelGGL(k_mc_tree, dim3(mc_blocks(first[l + 1] - first[l])), dim3(MC_THREADS), 0, st, G, first[l], first[l + 1] - first[l]);
    if (P > 0) hipLaunchKernelGGL(k_mc_spread, dim3(mc_blocks(P)), dim3(MC_THREADS), 0, st, S, P);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(h + oOut, d + oOut, pl.off - oOut, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    if (K > 0) {
        memcpy(out->TcwGBA_out16, h + oGba, (size_t)K * 64);
        memcpy(out->kf_marked, marked.data(), (size_t)K);
        if (out->kf_reached) memcpy(out->kf_reached, reached.data(), (size_t)K);
        for (int k = 0; k < K; k++) memcpy(out->Tcw_new16 + (size_t)k * 16, reached[k] ? h + oGba + (size_t)k * 64 : (const uint8_t *)(in->Tcw16 + (size_t)k * 16), 64);   // :707
    }
    if (P > 0) { memcpy(out->pos_out3, h + oPo, (size_t)P * 12); memcpy(out->status, h + oSt, (size_t)P * 4); }
    return ORBX_OK;
}
