// localmap_lockstep.cc — the text of the local map kernels' bodies (orb_slam2v2-1_amd/csrc/orbx_localmap_dev.h) compiled for the host and
// run as ONE lane per wave, one wave per workgroup, for tests/test_localmap_cpu.py: every output byte must equal the literal
// restatement tests/localmap_ref.py.  That pins the kernels' control flow - the vote, the compaction, the extension's three sub-steps and
// its break, the minimum of positions, the scans, the packing and the cleaning pass - without a GPU; what it cannot show - 64 lanes'
// ballots and shuffles, the LDS atomics and marks, the barriers, the global counter row, more than one workgroup on the walk - is
// tests/test_localmap_gpu.py's.  The frame runs TWICE on one state: exit status 4 if the cleaning pass left a word of the state
// that is not idle, 5 if the second run's bytes differ from the first's.
//   localmap_lockstep IN OUT
//       IN:  int32 K P nobs nlevels F ncov nchild N n_prev max_keyframes nbest | orbc_keyframe_t[K] | orbc_point_t[P] | int32 obs_off[P+1] |
//            orbc_observation_t[nobs] | float sf[nlevels] | int32 feat_off[K+1] | orbc_feature_t[F] | int32 parent[K] | cov_off[K+1] | cov[ncov] |
//            child_off[K+1] | child[nchild] | orbt_pointview_t[P] | uint8 desc[P][32] | int32 frame_points[N] | prev_kf[n_prev]
//       OUT: int32 empty_vote n_voted ref_kf ref_votes extension_end n_local_kf n_local_pts | frame_points[N] | holder[N] | ext_obs[N] |
//            local_kf[n_local_kf] | local_pts[m] | orbm_worldpoint_t[m] | uint8 mp_desc[m][32]
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "orbx.h"

#define ORBX_COVIS_HOST
#include "hip_lockstep.h"
// the built-ins of the kernels that hip_lockstep.h does not have, for a wave of one lane
static inline int __shfl(int v, int, int) { return v; }
static inline unsigned long long atomicMax(unsigned long long *p, unsigned long long v) { const unsigned long long old = *p; if (v > old) *p = v; return old; }
static inline int atomicMin(int *p, int v) { const int old = *p; if (v < old) *p = v; return old; }
static inline uint32_t atomicOr(uint32_t *p, uint32_t v) { const uint32_t old = *p; *p |= v; return old; }
static inline int __ffsll(long long v) { return __builtin_ffsll(v); }
#include "orbx_localmap_dev.h"

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n + 1);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char **argv) {
    if (argc != 3) { fprintf(stderr, "usage: localmap_lockstep IN OUT\n"); return 2; }
    FILE *f = fopen(argv[1], "rb");
    int32_t hd[11];
    if (!f || fread(hd, 4, 11, f) != 11) return 1;
    const int K = hd[0], P = hd[1], nobs = hd[2], nlevels = hd[3], NF = hd[4], ncov = hd[5], nchild = hd[6], N = hd[7], n_prev = hd[8];
    std::vector<orbc_keyframe_t> kf;
    std::vector<orbc_point_t> pts;
    std::vector<int32_t> off, foff, parent, coff, cov, hoff, child, fpts, prev;
    std::vector<orbc_observation_t> obs;
    std::vector<float> sf;
    std::vector<orbc_feature_t> feat;
    std::vector<orbt_pointview_t> views;
    std::vector<uint32_t> desc;   // words: the kernel copies a descriptor as eight of them
    if (!rd(f, kf, K) || !rd(f, pts, P) || !rd(f, off, P + 1) || !rd(f, obs, nobs) || !rd(f, sf, nlevels) || !rd(f, foff, K + 1) || !rd(f, feat, NF) ||
        !rd(f, parent, K) || !rd(f, coff, K + 1) || !rd(f, cov, ncov) || !rd(f, hoff, K + 1) || !rd(f, child, nchild) || !rd(f, views, P) ||
        !rd(f, desc, (size_t)P * 8) || !rd(f, fpts, N) || !rd(f, prev, n_prev)) return 1;
    fclose(f);
    // the snapshot as orbt_localmap_set_map packs it: the features' points alone
    std::vector<int32_t> featpt(NF + 1);
    for (int i = 0; i < NF; i++) featpt[i] = feat[i].point;
    LmMap M;
    M.T.kf = kf.data(); M.T.pts = pts.data(); M.T.obs_off = off.data(); M.T.obs = obs.data(); M.T.sf = sf.data(); M.T.K = K; M.T.P = P; M.T.nlevels = nlevels;
    M.feat_off = foff.data(); M.feat_pt = featpt.data(); M.parent = parent.data(); M.cov_off = coff.data(); M.cov = cov.data(); M.child_off = hoff.data();
    M.child = child.data(); M.views = views.data(); M.desc = (const uint8_t *)desc.data();

    // the handle's state, idle; the frame's block
    std::vector<int32_t> first(P + 1, LM_IDLE);
    std::vector<uint8_t> inframe(P + 1, 0);
    std::vector<orbc_feature_t> ffeat(N + 1);
    for (int i = 0; i < N; i++) { ffeat[i].point = fpts[i]; ffeat[i].octave = 0; ffeat[i].depth = 0.f; }
    std::vector<uint8_t> outs[2];
    for (int rep = 0; rep < 2; rep++) {
        // nothing of the frame's block is zero on entry but what the call itself zeroes
        std::vector<int32_t> counters(K + 1, 0), kf_start(K + 2, -77), rank(NF + 1, -77), tile_cnt(NF + 1, -77), fp(N + 1, -77), holder(N + 1, -77), ext(N + 1, -77),
            local_kf(K + 1, -77), local_pts(P + 1, -77);
        std::vector<orbm_worldpoint_t> wp(P + 1);
        std::vector<uint32_t> mpd((size_t)P * 8 + 1, 0xABABABABu);
        LmHead head;
        memset(&head, 0x55, sizeof head);
        LmFrame F;
        F.feat = ffeat.data(); F.prev_kf = prev.data(); F.N = N; F.n_prev = n_prev; F.max_keyframes = hd[9]; F.nbest = hd[10];
        F.counters = counters.data(); F.first = first.data(); F.inframe = inframe.data(); F.kf_start = kf_start.data(); F.rank = rank.data();
        F.tile_cnt = tile_cnt.data(); F.head = &head; F.fp = fp.data(); F.holder = holder.data(); F.ext_obs = ext.data(); F.local_kf = local_kf.data();
        F.local_pts = local_pts.data(); F.pts = wp.data(); F.mp_desc = (uint8_t *)mpd.data();
        // the launches of orbt_update_local_map, each grid as one workgroup (gridDim.x == 1: the strided loops cover everything)
        blockIdx.x = 0;
        lm_vote(M, F, counters.data());
        {
            std::vector<uint32_t> bits((size_t)(K + 31) / 32 + 1, 0xFFFFFFFFu);
            int sWave[1], sScan[1], sAny = -1, sLen = -1, sEnd = -1;
            unsigned long long sBest = ~0ull;
            lm_keyframes(M, F, bits.data(), sWave, sScan, &sAny, &sLen, &sEnd, &sBest);
        }
        int sWave[1], sScan[1];
        lm_first(M, F);
        lm_count(M, F, sWave);
        lm_scan(F, sScan);
        lm_emit(M, F, sWave);
        lm_holder(M, F);
        lm_clean(M, F);
        for (int p = 0; p < P; p++)
            if (first[p] != LM_IDLE || inframe[p] != 0) return 4;
        const int nk = head.n_local_kf, m = head.n_local_pts;
        if (nk < 0 || nk > K || m < 0 || m > P) return 6;
        const int32_t h7[7] = {head.empty_vote, head.n_voted, head.ref_kf, head.ref_votes, head.extension_end, nk, m};
        std::vector<uint8_t> &o = outs[rep];
        auto put = [&o](const void *p, size_t n) { const uint8_t *b = (const uint8_t *)p; o.insert(o.end(), b, b + n); };
        put(h7, sizeof h7); put(fp.data(), (size_t)N * 4); put(holder.data(), (size_t)N * 4); put(ext.data(), (size_t)N * 4); put(local_kf.data(), (size_t)nk * 4);
        put(local_pts.data(), (size_t)m * 4); put(wp.data(), (size_t)m * sizeof(orbm_worldpoint_t)); put(mpd.data(), (size_t)m * 32);
    }
    if (outs[0] != outs[1]) return 5;
    f = fopen(argv[2], "wb");
    if (!f) return 1;
    fwrite(outs[0].data(), 1, outs[0].size(), f);
    fclose(f);
    return 0;
}
