// orbx_covis_dev.h — the device code of orbx_covis.hip that needs no HIP header: the bodies of k_cov_count, k_cov_order (with its
// in-LDS sort), k_cull and k_normals.  orbx_covis.hip wraps them in kernels; tests/cpp/covis_lockstep.cc compiles the same text for
// the host with ORBX_COVIS_HOST defined, as ONE lane per wave and one wave per workgroup (tests/cpp/hip_lockstep.h comes first, and
// the program supplies the two built-ins that header lacks: __shfl and the 64-bit atomicMax).
// Lists longer than ORBC_SORT_LDS take the radix core of orbx_cloud_dev.h, which is HIP code and stays in orbx_covis.hip.
//
// All integer results are sums, ballots and maxima of integers: no order of arrival can change them.  The one float routine,
// cov_normal, is one thread walking one list in list order.
#pragma once
#include <math.h>
#include <stdint.h>
#include "orbx.h"
#include "orbx_div_rn.h"

#ifdef ORBX_COVIS_HOST
#define COV_WAVE 1
#define COV_COUNT_THREADS 1
#define COV_ORDER_THREADS 1
#define COV_CULL_THREADS 1
#else
#define COV_WAVE 64
#define COV_COUNT_THREADS 512
#define COV_ORDER_THREADS 256    // = CL_THREADS: the radix core's workgroup
#define COV_CULL_THREADS 1024
#endif
#define COV_NORMAL_THREADS 256

// the table as the kernels address it
struct CovTable { const orbc_keyframe_t *kf; const orbc_point_t *pts; const int32_t *obs_off; const orbc_observation_t *obs; const float *sf; int32_t K, P, nlevels; };
struct CovQueries { const int32_t *query_kf, *feat_off; const orbc_feature_t *feat; int32_t Q; };

__device__ __forceinline__ int cov_lane() { return (int)(threadIdx.x % COV_WAVE); }
__device__ __forceinline__ int cov_wave() { return (int)(threadIdx.x / COV_WAVE); }
__device__ __forceinline__ unsigned long long cov_lanes_below() { return (1ull << cov_lane()) - 1ull; }

// ---- k_cov_count: src/KeyFrame.cc:303-321 for one query.  A wave loads COV_WAVE features at once (one per lane: the feature, its
// point's flag and the bounds of its list), then serves them one after the other with its lanes on the observations.
// tab: K counters, zero on entry, in LDS or in the query's row of the global block
__device__ __forceinline__ void cov_count_query(const CovTable &T, const orbc_feature_t *feat, int f0, int f1, int s, int32_t *tab) {
    const int lane = cov_lane(), nw = COV_COUNT_THREADS / COV_WAVE;
    for (int base = f0 + cov_wave() * COV_WAVE; base < f1; base += nw * COV_WAVE) {
        const int f = base + lane;
        int lo = 0, hi = 0;
        if (f < f1) {
            const int p = feat[f].point;
            if (p >= 0 && !T.pts[p].bad) { lo = T.obs_off[p]; hi = T.obs_off[p + 1]; }   // :307-311
        }
        const int m = f1 - base < COV_WAVE ? f1 - base : COV_WAVE;
        for (int j = 0; j < m; j++) {
            const int l = __shfl(lo, j, COV_WAVE), h = __shfl(hi, j, COV_WAVE);
            for (int o = l + lane; o < h; o += COV_WAVE) {
                const int k = T.obs[o].kf;
                if (k != s) atomicAdd(&tab[k], 1);   // :317-319
            }
        }
    }
}

// ---- k_cov_order: src/KeyFrame.cc:324-362 for one query from its counters.  A key is weight << sb | slot, sb = the bits of K - 1:
// ascending keys are the reference's sort on (weight, pointer), and the list is its reverse.
// Step 1: how many counters reach th, and the largest (counter, first slot) among the counters above 0.  sCnt, sBest: LDS words
__device__ __forceinline__ void cov_order_scan(const int32_t *row, int K, int th, int *sCnt, unsigned long long *sBest) {
    if (threadIdx.x == 0) { *sCnt = 0; *sBest = 0ull; }
    __syncthreads();
    int cnt = 0;
    unsigned long long best = 0ull;
    for (int k = threadIdx.x; k < K; k += COV_ORDER_THREADS) {
        const int c = row[k];
        if (c >= th) cnt++;
        const unsigned long long key = ((unsigned long long)(uint32_t)c << 32) | (uint32_t)(0x7FFFFFFF - k);   // the max over keys: largest counter, then smallest slot (:337-341: `>` keeps the first)
        if (c > 0 && key > best) best = key;
    }
    if (cnt) atomicAdd(sCnt, cnt);
    if (best) atomicMax(sBest, best);
    __syncthreads();
}
// Step 2: the keys of the counters that reach th, in slot order, to dst[0..n).  sWave: one int per wave of LDS
__device__ __forceinline__ void cov_order_compact(const int32_t *row, int K, int th, int sb, unsigned long long *dst, int *sWave) {
    const int nw = COV_ORDER_THREADS / COV_WAVE;
    int run = 0;
    for (int k0 = 0; k0 < K; k0 += COV_ORDER_THREADS) {
        const int k = k0 + (int)threadIdx.x;
        const int c = k < K ? row[k] : 0;
        const bool flag = k < K && c >= th;
        const unsigned long long m = __ballot(flag);
        if (cov_lane() == 0) sWave[cov_wave()] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < nw; w++) { const int t = sWave[w]; if (w < cov_wave()) before += t; total += t; }
        if (flag) dst[run + before + __popcll(m & cov_lanes_below())] = ((unsigned long long)(uint32_t)c << sb) | (unsigned long long)(uint32_t)k;
        run += total;
        __syncthreads();
    }
}
// Step 3, lists up to ORBC_SORT_LDS: a bitonic network over s[0..N), N the power of two >= n, the tail padded with 0 (a key is > 0:
// th >= 1).  Descending on return
__device__ __forceinline__ void cov_sort_lds(unsigned long long *s, int n) {
    int N = 1;
    while (N < n) N <<= 1;
    for (int i = n + (int)threadIdx.x; i < N; i += COV_ORDER_THREADS) s[i] = 0ull;
    __syncthreads();
    for (int k = 2; k <= N; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < N; i += COV_ORDER_THREADS) {
                const int x = i ^ j;
                if (x > i) {
                    const unsigned long long a = s[i], b = s[x];
                    if ((i & k) == 0 ? a < b : a > b) { s[i] = b; s[x] = a; }
                }
            }
            __syncthreads();
        }
}
// Step 4: the first min(n, cap) entries; src descending (rev = 0) or ascending (rev = 1)
__device__ __forceinline__ void cov_order_emit(const unsigned long long *src, int n, int rev, int sb, int cap, int32_t *ids, int32_t *weights) {
    const int m = n < cap ? n : cap;
    for (int i = threadIdx.x; i < m; i += COV_ORDER_THREADS) {
        const unsigned long long key = src[rev ? n - 1 - i : i];
        ids[i] = (int32_t)(key & ((1ull << sb) - 1ull));
        weights[i] = (int32_t)(key >> sb);
    }
}
// The single entry of a query none of whose counters reaches th (:349-353); best as cov_order_scan left it
__device__ __forceinline__ void cov_order_single(unsigned long long best, int cap, int32_t *ids, int32_t *weights, int32_t *n) {
    if (threadIdx.x != 0) return;
    *n = best ? 1 : 0;   // every counter 0: the early return (:324-325)
    if (best && cap > 0) { ids[0] = 0x7FFFFFFF - (int32_t)(best & 0xFFFFFFFFull); weights[0] = (int32_t)(best >> 32); }
}

// ---- k_cull: src/LocalMapping.cc:640-704, the queries in order, by ONE workgroup with all its waves on one keyframe.  What the
// reference's SetBadFlag / EraseObservation / MapPoint::SetBadFlag leave behind is a function of the set C of keyframes culled so
// far (include/orbx.h), kept as one bit per slot in LDS; a point's state is re-derived from its list and C wherever it is read.
__device__ __forceinline__ bool cov_bit(const uint32_t *bits, int k) { return (bits[k >> 5] >> (k & 31)) & 1u; }
// lost / nObs of a point by one thread (the final flags)
__device__ __forceinline__ bool cov_point_bad(const CovTable &T, const uint32_t *bits, int p) {
    if (T.pts[p].bad) return true;
    int lost = 0, nobs = 0;
    for (int o = T.obs_off[p]; o < T.obs_off[p + 1]; o++) {
        const orbc_observation_t ob = T.obs[o];
        if (cov_bit(bits, ob.kf)) lost++;
        else nobs += ob.stereo ? 2 : 1;
    }
    return lost >= 1 && nobs <= 2;   // src/MapPoint.cc:131-148: EraseObservation sets the flag when nObs <= 2 after an erase
}
// bits: (K + 31) / 32 words of LDS; sM, sR: LDS words
__device__ __forceinline__ void cov_cull(const CovTable &T, const CovQueries &Qs, int monocular, int th_obs, int32_t *n_mps, int32_t *n_red,
                                         int32_t *verdict, uint8_t *point_bad, uint32_t *bits, int *sM, int *sR) {
    const int lane = cov_lane(), nw = COV_CULL_THREADS / COV_WAVE;
    for (int w = threadIdx.x; w < (T.K + 31) / 32; w += COV_CULL_THREADS) bits[w] = 0u;
    __syncthreads();
    for (int q = 0; q < Qs.Q; q++) {
        const int s = Qs.query_kf[q];
        const orbc_keyframe_t me = T.kf[s];
        if (me.id == 0) {   // :651-652
            if (threadIdx.x == 0) { n_mps[q] = 0; n_red[q] = 0; verdict[q] = 0; }
            continue;
        }
        if (threadIdx.x == 0) { *sM = 0; *sR = 0; }
        __syncthreads();
        const int f0 = Qs.feat_off[q], f1 = Qs.feat_off[q + 1];
        int myM = 0, myR = 0;   // wave-uniform
        for (int base = f0 + cov_wave() * COV_WAVE; base < f1; base += nw * COV_WAVE) {
            const int f = base + lane;
            int lo = 0, hi = 0, oct = 0;
            bool cand = false;
            if (f < f1) {
                const orbc_feature_t ft = Qs.feat[f];
                if (ft.point >= 0 && !T.pts[ft.point].bad && (monocular || !(ft.depth > me.th_depth || ft.depth < 0))) {   // :662-670
                    cand = true; lo = T.obs_off[ft.point]; hi = T.obs_off[ft.point + 1]; oct = ft.octave;
                }
            }
            const unsigned long long cm = __ballot(cand);
            const int m = f1 - base < COV_WAVE ? f1 - base : COV_WAVE;
            for (int j = 0; j < m; j++) {
                if (!((cm >> j) & 1ull)) continue;
                const int l = __shfl(lo, j, COV_WAVE), h = __shfl(hi, j, COV_WAVE), oc = __shfl(oct, j, COV_WAVE);
                int lost = 0, nobs = 0, others = 0;
                for (int o0 = l; o0 < h; o0 += COV_WAVE) {
                    const int o = o0 + lane;
                    bool gone = false, live = false, st = false, oth = false;
                    if (o < h) {
                        const orbc_observation_t ob = T.obs[o];
                        gone = cov_bit(bits, ob.kf);
                        live = !gone;
                        st = live && ob.stereo;
                        oth = live && ob.kf != s && (int)ob.octave <= oc + 1;   // :681-685
                    }
                    lost += __popcll(__ballot(gone));
                    nobs += __popcll(__ballot(live)) + __popcll(__ballot(st));
                    others += __popcll(__ballot(oth));
                }
                if (lost >= 1 && nobs <= 2) continue;   // the point went bad when a culled keyframe left it: isBad() (:664)
                myM++;                                      // :672
                if (nobs > th_obs && others >= th_obs) myR++;   // :673-695
            }
        }
        if (lane == 0) { if (myM) atomicAdd(sM, myM); if (myR) atomicAdd(sR, myR); }
        __syncthreads();
        if (threadIdx.x == 0) {
            const int nM = *sM, nR = *sR;
            const int v = (double)nR > 0.9 * (double)nM ? (me.not_erase ? 2 : 1) : 0;   // :701; src/KeyFrame.cc:460-464
            n_mps[q] = nM; n_red[q] = nR; verdict[q] = v;
            if (v == 1) bits[s >> 5] |= 1u << (s & 31);
        }
        __syncthreads();
    }
    if (point_bad)
        for (int p = threadIdx.x; p < T.P; p += COV_CULL_THREADS) point_bad[p] = cov_point_bad(T, bits, p) ? 1 : 0;
}

// ---- k_normals: src/MapPoint.cc:340-383 for one point, the arithmetic of host/frame_shim.h's MapPoint::UpdateNormalAndDepth.
// pos: the point's position; ow(k): GetCameraCenter() of slot k as this point sees it (the table's for k_normals; orbx_mapcorrect_dev.h
// hands in the one that LoopClosing::CorrectLoop's sequential loop would have left there)
template <class OwFn>
__device__ __forceinline__ orbc_normal_t cov_normal_at(const CovTable &T, int p, const float *pos, OwFn ow) {
    orbc_normal_t r;
    r.normal[0] = 0.f; r.normal[1] = 0.f; r.normal[2] = 0.f; r.max_distance = 0.f; r.min_distance = 0.f; r.status = ORBC_NORMAL_OK;
    orbc_point_t pt = T.pts[p];
    pt.pos[0] = pos[0]; pt.pos[1] = pos[1]; pt.pos[2] = pos[2];
    const int lo = T.obs_off[p], hi = T.obs_off[p + 1];
    if (pt.bad) { r.status = ORBC_NORMAL_BAD; return r; }
    if (hi == lo) { r.status = ORBC_NORMAL_NO_OBSERVATION; return r; }
    float normal[3] = {0.f, 0.f, 0.f};
    int n = 0, level = -1;
    for (int o = lo; o < hi; o++) {
        const orbc_observation_t ob = T.obs[o];
        const float *Owi = ow(ob.kf);
        float normali[3];
        double s = 0;
        for (int k = 0; k < 3; k++) { normali[k] = pt.pos[k] - Owi[k]; s += (double)normali[k] * (double)normali[k]; }
        const float inv = (float)(1.0 / sqrt(s));
        for (int k = 0; k < 3; k++) normal[k] = normali[k] * inv + normal[k];   // a multiply, then an add: the build has -ffp-contract=off
        n++;
        if (ob.kf == pt.ref_kf) level = ob.octave;
    }
    if (level < 0) { r.status = ORBC_NORMAL_NO_REFERENCE; return r; }
    const float *Or = ow(pt.ref_kf);
    double s = 0;
    for (int k = 0; k < 3; k++) { const float d = pt.pos[k] - Or[k]; s += (double)d * (double)d; }
    const float dist = (float)sqrt(s);
    r.max_distance = dist * T.sf[level];
    r.min_distance = (float)orbx_div_rn((double)r.max_distance, (double)T.sf[T.nlevels - 1]);   // two floats' quotient rounded to double, then to float, is the correctly rounded float quotient (53 >= 2 * 24 + 2)
    for (int k = 0; k < 3; k++) r.normal[k] = (float)((double)normal[k] * (1.0 / n));
    return r;
}
__device__ __forceinline__ orbc_normal_t cov_normal(const CovTable &T, int p) {
    return cov_normal_at(T, p, T.pts[p].pos, [&T](int k) { return T.kf[k].Ow; });
}
