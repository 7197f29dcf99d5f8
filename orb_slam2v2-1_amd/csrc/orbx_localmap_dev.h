// orbx_localmap_dev.h — the device code of orbx_localmap.hip that needs no HIP header: the bodies of the k_lm_* kernels, Tracking::UpdateLocalMap
// (reference: src/Tracking.cc:1340-1484) over the resident snapshot.  orbx_localmap.hip wraps them in kernels; tests/cpp/localmap_lockstep.cc
// compiles the same text for the host with ORBX_COVIS_HOST defined, as ONE lane per wave and one wave per workgroup (tests/cpp/hip_lockstep.h
// comes first, and the program supplies the built-ins that header lacks).
//
// Every result is a sum, a ballot, a maximum or a minimum of integers, or a copied float: no order of arrival can change it.  The one
// sequential part, the extension of the keyframe list, is ONE wave that keeps the list's length in a register and the marks in LDS.
#pragma once
#include "orbx_covis_dev.h"

#ifdef ORBX_COVIS_HOST
#define LM_KF_THREADS 1
#define LM_THREADS 1
#else
#define LM_KF_THREADS 256
#define LM_THREADS 256      // the workgroup of the kernels over the walk, and their tile
#endif
#define LM_IDLE 0x7FFFFFFF  // first[p] of a point that no position of the walk names; a position is below the total feature count

// the snapshot as the kernels address it: the a33 table, every keyframe's point indices, the graph, the points' views and descriptors
struct LmMap { CovTable T; const int32_t *feat_off, *feat_pt, *parent, *cov_off, *cov, *child_off, *child; const orbt_pointview_t *views; const uint8_t *desc; };
// what the launches of one frame hand each other in device memory; the first 32 bytes of the download
struct LmHead { int32_t n_local_kf, n_local_pts, walk, empty_vote, n_voted, ref_kf, ref_votes, extension_end; };
// one frame.  feat: the frame's points as a33 feature records (only .point is set).  first [P] (LM_IDLE) and inframe [P] (0) are the
// handle's state, idle on entry and on return; kf_start [n_local_kf + 1]: where each local keyframe's features start in the
// concatenated walk; rank [walk]: the local index of the point a winning position names; tile_cnt [tiles of the walk]
struct LmFrame { const orbc_feature_t *feat; const int32_t *prev_kf; int32_t N, n_prev, max_keyframes, nbest;
                 int32_t *counters, *first; uint8_t *inframe; int32_t *kf_start, *rank, *tile_cnt; LmHead *head;
                 int32_t *fp, *holder, *ext_obs, *local_kf, *local_pts; orbm_worldpoint_t *pts; uint8_t *mp_desc; };

__device__ __forceinline__ bool lm_bit(const volatile uint32_t *bits, int k) { return (bits[k >> 5] >> (k & 31)) & 1u; }

// ---- k_lm_vote: steps 0 and 1 (:1380-1396).  fp and the in-frame marks by one thread per feature; the counters by cov_count_query
// with no slot left out.  tab: K counters, zero on entry
__device__ __forceinline__ void lm_vote(const LmMap &M, const LmFrame &F, int32_t *tab) {
    for (int i = threadIdx.x; i < F.N; i += COV_COUNT_THREADS) {
        int p = F.feat[i].point;
        if (p >= 0 && M.T.pts[p].bad) p = -1;   // :1391-1394
        F.fp[i] = p;
        if (p >= 0) F.inframe[p] = 1;           // the same byte from every feature that names p
    }
    cov_count_query(M.T, F.feat, 0, F.N, -1, tab);
}

// ---- k_lm_keyframes: steps 2 to 4 by ONE workgroup, then the walk's offsets.
// The first candidate of cand[0..n) that is neither bad nor marked, by one wave with its lanes on the candidates; -1: none
__device__ __forceinline__ int lm_first_free(const LmMap &M, const int32_t *cand, int n, const volatile uint32_t *bits) {
    for (int c0 = 0; c0 < n; c0 += COV_WAVE) {
        const int c = c0 + cov_lane();
        int k = -1;
        bool ok = false;
        if (c < n) { k = cand[c]; ok = !M.T.kf[k].bad && !lm_bit(bits, k); }
        const unsigned long long m = __ballot(ok);
        if (m) return __shfl(k, __ffsll((long long)m) - 1, COV_WAVE);
    }
    return -1;
}
// push_back + the mark; every lane keeps the length
__device__ __forceinline__ int lm_append(const LmFrame &F, volatile uint32_t *bits, int len, int k) {
    if (cov_lane() == 0) { F.local_kf[len] = k; bits[k >> 5] |= 1u << (k & 31); }
    return len + 1;
}
// bits: (K + 31) / 32 words of LDS; sWave: one int per wave; sScan: LM_KF_THREADS ints; sAny, sLen, sEnd, sBest: LDS words
__device__ __forceinline__ void lm_keyframes(const LmMap &M, const LmFrame &F, uint32_t *bits, int *sWave, int *sScan, int *sAny, int *sLen, int *sEnd,
                                             unsigned long long *sBest) {
    const int K = M.T.K, nw = LM_KF_THREADS / COV_WAVE, tid = (int)threadIdx.x;
    for (int w = tid; w < (K + 31) / 32; w += LM_KF_THREADS) bits[w] = 0u;
    if (tid == 0) { *sAny = 0; *sBest = 0ull; *sLen = 0; *sEnd = ORBT_END_RAN_OUT; }
    __syncthreads();
    // step 3 (:1408-1423): the voted, not bad slots in slot order (a ballot compaction) and the largest (counter, first slot) among them
    int run = 0;
    bool any = false;
    unsigned long long best = 0ull;
    for (int k0 = 0; k0 < K; k0 += LM_KF_THREADS) {
        const int k = k0 + tid;
        const int c = k < K ? F.counters[k] : 0;
        if (c > 0) any = true;
        const bool flag = c > 0 && !M.T.kf[k].bad;   // :1412-1413
        if (flag) {
            const unsigned long long key = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)(0x7FFFFFFF - k);   // `>` keeps the first (:1415)
            if (key > best) best = key;
            atomicOr(&bits[k >> 5], 1u << (k & 31));   // :1422
        }
        const unsigned long long m = __ballot(flag);
        if (cov_lane() == 0) sWave[cov_wave()] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < nw; w++) { const int t = sWave[w]; if (w < cov_wave()) before += t; total += t; }
        if (flag) F.local_kf[run + before + __popcll(m & cov_lanes_below())] = k;
        run += total;
        __syncthreads();
    }
    if (any) atomicAdd(sAny, 1);
    if (best) atomicMax(sBest, best);
    __syncthreads();
    const int S = run;
    const bool empty = *sAny == 0;   // keyframeCounter.empty() (:1398): a bad keyframe's counter counts
    if (empty) {
        for (int j = tid; j < F.n_prev; j += LM_KF_THREADS) F.local_kf[j] = F.prev_kf[j];   // the early return: the list stays
        if (tid == 0) *sLen = F.n_prev;
    } else if (cov_wave() == 0) {
        // step 4 (:1427-1477): one wave; j walks the first-stage entries only
        volatile uint32_t *vb = bits;
        int len = S, end = ORBT_END_RAN_OUT;
        for (int j = 0; j < S; j++) {
            if (len > F.max_keyframes) { end = ORBT_END_LENGTH; break; }   // :1430
            const int kf = F.local_kf[j];
            int nc = M.cov_off[kf + 1] - M.cov_off[kf];
            if (nc > F.nbest) nc = F.nbest;                                 // GetBestCovisibilityKeyFrames(10)
            int a = lm_first_free(M, M.cov + M.cov_off[kf], nc, vb);        // :1437-1449
            if (a >= 0) len = lm_append(F, vb, len, a);
            a = lm_first_free(M, M.child + M.child_off[kf], M.child_off[kf + 1] - M.child_off[kf], vb);   // :1451-1464
            if (a >= 0) len = lm_append(F, vb, len, a);
            const int pa = M.parent[kf];
            if (pa >= 0 && !lm_bit(vb, pa)) {   // :1466-1475: no isBad(), and the break leaves THIS loop
                len = lm_append(F, vb, len, pa);
                end = ORBT_END_PARENT;
                break;
            }
        }
        if (cov_lane() == 0) { *sLen = len; *sEnd = end; }
    }
    __syncthreads();
    // the concatenated walk of step 5: kf_start[j] = the features of the local keyframes before the j-th (a scan, LM_KF_THREADS at a time)
    const int len = *sLen;
    int walk = 0;
    for (int j0 = 0; j0 < len; j0 += LM_KF_THREADS) {
        const int j = j0 + tid;
        int v = 0;
        if (j < len) { const int kf = F.local_kf[j]; v = M.feat_off[kf + 1] - M.feat_off[kf]; }
        sScan[tid] = v;
        __syncthreads();
        for (int d = 1; d < LM_KF_THREADS; d <<= 1) {
            const int t = tid >= d ? sScan[tid - d] : 0;
            __syncthreads();
            sScan[tid] += t;
            __syncthreads();
        }
        if (j < len) F.kf_start[j] = walk + sScan[tid] - v;
        walk += sScan[LM_KF_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) {
        F.kf_start[len] = walk;
        LmHead h;
        const unsigned long long b = *sBest;
        h.n_local_kf = len; h.n_local_pts = 0; h.walk = walk; h.empty_vote = empty ? 1 : 0; h.n_voted = empty ? 0 : S;
        h.ref_kf = b ? 0x7FFFFFFF - (int32_t)(b & 0xFFFFFFFFull) : -1; h.ref_votes = (int32_t)(b >> 32); h.extension_end = *sEnd;
        *F.head = h;
    }
}

// ---- the kernels over the walk.  The point a position names, or -1 for a NULL slot or a bad point (:1362-1366)
__device__ __forceinline__ int lm_point_at(const LmMap &M, const LmFrame &F, int nkf, int pos) {
    int lo = 0, hi = nkf - 1;   // the last j with kf_start[j] <= pos: a keyframe without features owns no position
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (F.kf_start[mid] <= pos) lo = mid; else hi = mid - 1;
    }
    const int p = M.feat_pt[M.feat_off[F.local_kf[lo]] + (pos - F.kf_start[lo])];
    return p >= 0 && !M.T.pts[p].bad ? p : -1;
}
// k_lm_first: a point is listed where the walk meets it first: the minimum of its positions
__device__ __forceinline__ void lm_first(const LmMap &M, const LmFrame &F) {
    const int nkf = F.head->n_local_kf, walk = F.head->walk;
    for (int pos = blockIdx.x * LM_THREADS + threadIdx.x; pos < walk; pos += gridDim.x * LM_THREADS) {
        const int p = lm_point_at(M, F, nkf, pos);
        if (p >= 0) atomicMin(&F.first[p], pos);
    }
}
// k_lm_count: how many positions of each tile won.  sWave: one int per wave
__device__ __forceinline__ void lm_count(const LmMap &M, const LmFrame &F, int *sWave) {
    const int nkf = F.head->n_local_kf, walk = F.head->walk, tiles = (walk + LM_THREADS - 1) / LM_THREADS, nw = LM_THREADS / COV_WAVE;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int pos = t * LM_THREADS + (int)threadIdx.x;
        bool win = false;
        if (pos < walk) { const int p = lm_point_at(M, F, nkf, pos); win = p >= 0 && F.first[p] == pos; }
        const unsigned long long m = __ballot(win);
        if (cov_lane() == 0) sWave[cov_wave()] = __popcll(m);
        __syncthreads();
        if (threadIdx.x == 0) { int s = 0; for (int w = 0; w < nw; w++) s += sWave[w]; F.tile_cnt[t] = s; }
        __syncthreads();
    }
}
// k_lm_scan: ONE workgroup turns the tiles' counts into their offsets; the total is n_local_pts.  sScan: LM_THREADS ints
__device__ __forceinline__ void lm_scan(const LmFrame &F, int *sScan) {
    const int walk = F.head->walk, tiles = (walk + LM_THREADS - 1) / LM_THREADS, tid = (int)threadIdx.x;
    int run = 0;
    for (int t0 = 0; t0 < tiles; t0 += LM_THREADS) {
        const int t = t0 + tid, v = t < tiles ? F.tile_cnt[t] : 0;
        sScan[tid] = v;
        __syncthreads();
        for (int d = 1; d < LM_THREADS; d <<= 1) {
            const int x = tid >= d ? sScan[tid - d] : 0;
            __syncthreads();
            sScan[tid] += x;
            __syncthreads();
        }
        if (t < tiles) F.tile_cnt[t] = run + sScan[tid] - v;
        run += sScan[LM_THREADS - 1];
        __syncthreads();
    }
    if (tid == 0) F.head->n_local_pts = run;
}
// k_lm_emit: the winners in walk order (step 5) and their records (step 6).  A record is what SearchLocalPointsHIP packs
__device__ __forceinline__ void lm_emit(const LmMap &M, const LmFrame &F, int *sWave) {
    const int nkf = F.head->n_local_kf, walk = F.head->walk, tiles = (walk + LM_THREADS - 1) / LM_THREADS;
    for (int t = blockIdx.x; t < tiles; t += gridDim.x) {
        const int pos = t * LM_THREADS + (int)threadIdx.x;
        int p = -1;
        if (pos < walk) { p = lm_point_at(M, F, nkf, pos); if (p >= 0 && F.first[p] != pos) p = -1; }
        const unsigned long long m = __ballot(p >= 0);
        if (cov_lane() == 0) sWave[cov_wave()] = __popcll(m);
        __syncthreads();
        int before = 0;
        for (int w = 0; w < cov_wave(); w++) before += sWave[w];
        if (p >= 0) {
            const int j = F.tile_cnt[t] + before + __popcll(m & cov_lanes_below());
            F.local_pts[j] = p;
            F.rank[pos] = j;
            const orbt_pointview_t v = M.views[p];
            const bool valid = !F.inframe[p];   // mnLastFrameSeen == mCurrentFrame.mnId (:1315); a listed point is not bad
            orbm_worldpoint_t r;
            r.valid = valid ? 1 : 0;
            r.wx = valid ? M.T.pts[p].pos[0] : 0.f; r.wy = valid ? M.T.pts[p].pos[1] : 0.f; r.wz = valid ? M.T.pts[p].pos[2] : 0.f;
            r.nx = valid ? v.normal[0] : 0.f; r.ny = valid ? v.normal[1] : 0.f; r.nz = valid ? v.normal[2] : 0.f;
            r.max_distance = valid ? v.max_distance : 0.f; r.min_distance = valid ? v.min_distance : 0.f;
            r.observations = v.observations;
            F.pts[j] = r;
            const uint32_t *src = (const uint32_t *)(M.desc + (size_t)32 * p);
            uint32_t *dst = (uint32_t *)(F.mp_desc + (size_t)32 * j);
            for (int w = 0; w < 8; w++) dst[w] = valid ? src[w] : 0u;
        }
        __syncthreads();
    }
}
// k_lm_holder: the frame's own slots (step 6)
__device__ __forceinline__ void lm_holder(const LmMap &M, const LmFrame &F) {
    for (int i = blockIdx.x * LM_THREADS + threadIdx.x; i < F.N; i += gridDim.x * LM_THREADS) {
        const int p = F.fp[i];
        int h = -1, e = 0;
        if (p >= 0) {
            const int f = F.first[p];
            if (f == LM_IDLE) { h = -2; e = M.views[p].observations; }
            else h = F.rank[f];
        }
        F.holder[i] = h; F.ext_obs[i] = e;
    }
}
// k_lm_clean: the state back to idle over the positions and the features that touched it, so that a frame's cost does not grow with P
__device__ __forceinline__ void lm_clean(const LmMap &M, const LmFrame &F) {
    const int nkf = F.head->n_local_kf, walk = F.head->walk;
    for (int pos = blockIdx.x * LM_THREADS + threadIdx.x; pos < walk; pos += gridDim.x * LM_THREADS) {
        const int p = lm_point_at(M, F, nkf, pos);
        if (p >= 0) F.first[p] = LM_IDLE;
    }
    for (int i = blockIdx.x * LM_THREADS + threadIdx.x; i < F.N; i += gridDim.x * LM_THREADS) {
        const int p = F.fp[i];
        if (p >= 0) F.inframe[p] = 0;
    }
}
