// mapcorrect_lockstep.cc — the text of the loop map correction kernels' bodies (orb_slam2v2-1_amd/csrc/orbx_mapcorrect_dev.h) and of the
// spread's graph work (orbx_mapcorrect_plan.h) compiled for the host and run as ONE thread per workgroup, for tests/test_mapcorrect_cpu.py:
// every output byte must equal the literal restatement tests/mapcorrect_ref.py.  That pins the arithmetic of the five bodies, the
// owner's minimum, the camera-centre rule of a corrected point's normal and the levels of the tree without a GPU; what it cannot show -
// 256 threads and more than one workgroup, the atomics between them, the staging block - is tests/test_mapcorrect_gpu.py's.
// Every buffer a kernel writes starts filled with a pattern, not zero.
//   mapcorrect_lockstep loop IN OUT
//       IN:  int32 K P nobs nlevels Q nfeat cur | orbc_keyframe_t[K] | orbc_point_t[P] | int32 obs_off[P+1] | orbc_observation_t[nobs] | float sf[nlevels] |
//            int32 query_kf[Q] | feat_off[Q+1] | orbc_feature_t[nfeat] | float Tiw[Q][16] | orbg_sim3_t Scw
//       OUT: orbg_sim3_t corrected[Q] | non_corrected[Q] | float Tiw_new[Q][16] | Ow_new[Q][3] | pos[P][3] | int32 corrected_ref[P] | orbc_normal_t[P]
//   mapcorrect_lockstep spread IN OUT
//       IN:  int32 K P nchild norigins | float Tcw[K][16] | TcwGBA[K][16] | uint8 kf_in_gba[K] | int32 child_off[K+1] | child[nchild] | origins[norigins] |
//            float pos[P][3] | posGBA[P][3] | uint8 pt_in_gba[P] | int32 ref_kf[P] | uint8 bad[P]
//       OUT: float Tcw_new[K][16] | TcwGBA[K][16] | uint8 kf_marked[K] | kf_reached[K] | float pos[P][3] | int32 status[P] | int32 levels
//   exit status 3: the graph work reported an argument error
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
#include "orbx_mapcorrect_dev.h"
#include "orbx_mapcorrect_plan.h"

template <typename T> static bool rd(FILE *f, std::vector<T> &v, size_t n) {
    v.resize(n + 1);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T> static void put(std::vector<uint8_t> &o, const std::vector<T> &v, size_t n) {
    const uint8_t *b = (const uint8_t *)v.data();
    o.insert(o.end(), b, b + n * sizeof(T));
}
static int write_out(const char *path, const std::vector<uint8_t> &o) {
    FILE *f = fopen(path, "wb");
    if (!f) return 1;
    fwrite(o.data(), 1, o.size(), f);
    fclose(f);
    return 0;
}

static int run_loop(FILE *f, const char *outp) {
    int32_t hd[7];
    if (fread(hd, 4, 7, f) != 7) return 1;
    const int K = hd[0], P = hd[1], nobs = hd[2], nlevels = hd[3], Q = hd[4], nfeat = hd[5], cur = hd[6];
    std::vector<orbc_keyframe_t> kf;
    std::vector<orbc_point_t> pts;
    std::vector<int32_t> off, qk, foff;
    std::vector<orbc_observation_t> obs;
    std::vector<float> sf, Tiw;
    std::vector<orbc_feature_t> feat;
    std::vector<orbg_sim3_t> Scw;
    if (!rd(f, kf, K) || !rd(f, pts, P) || !rd(f, off, P + 1) || !rd(f, obs, nobs) || !rd(f, sf, nlevels) || !rd(f, qk, Q) || !rd(f, foff, Q + 1) ||
        !rd(f, feat, nfeat) || !rd(f, Tiw, (size_t)Q * 16) || !rd(f, Scw, 1)) return 1;
    CovTable T;
    T.kf = kf.data(); T.pts = pts.data(); T.obs_off = off.data(); T.obs = obs.data(); T.sf = sf.data(); T.K = K; T.P = P; T.nlevels = nlevels;
    CovQueries Qs;
    Qs.query_kf = qk.data(); Qs.feat_off = foff.data(); Qs.feat = feat.data(); Qs.Q = Q;
    // what orbr_correct_loop's packing pass adds
    std::vector<int32_t> qpos(K + 1, -1);
    int curPos = -1;
    for (int q = 0; q < Q; q++) { qpos[qk[q]] = q; if (qk[q] == cur) curPos = q; }
    if (curPos < 0) return 3;
    orbg_sim3_t junk;
    memset(&junk, 0x55, sizeof junk);
    std::vector<orbg_sim3_t> corrected(Q + 1, junk), non_corrected(Q + 1, junk), inv(Q + 1, junk);
    std::vector<float> Tn((size_t)Q * 16 + 1, -77.f), Own((size_t)Q * 3 + 1, -77.f), pos((size_t)P * 3 + 1, -77.f);
    std::vector<int32_t> owner(P + 1, -77), ref(P + 1, -77);
    orbc_normal_t nj;
    memset(&nj, 0x55, sizeof nj);
    std::vector<orbc_normal_t> normals(P + 1, nj);
    McLoop L;
    L.Tiw = Tiw.data(); L.Scw = Scw[0]; L.Q = Q; L.cur_pos = curPos; L.corrected = corrected.data(); L.non_corrected = non_corrected.data();
    L.corrected_inv = inv.data(); L.Tiw_new = Tn.data(); L.Ow_new = Own.data();
    McPoints M;
    M.qpos = qpos.data(); M.query_kf = qk.data(); M.owner = owner.data(); M.non_corrected = non_corrected.data(); M.corrected_inv = inv.data();
    M.Ow_new = Own.data(); M.pos = pos.data(); M.corrected_ref = ref.data(); M.normals = normals.data();
    // the three launches of orbr_correct_loop, each grid as one workgroup of one thread (the strided loops cover everything)
    blockIdx.x = 0;
    { MC_FOR(q, L.Q) mc_sim3(L, q); MC_FOR(p, P) owner[p] = MC_NO_OWNER; }
    { MC_FOR(i, nfeat) mc_owner(T, Qs, i, owner.data()); }
    { MC_FOR(p, T.P) mc_point(T, M, p); }
    std::vector<uint8_t> o;
    put(o, corrected, Q); put(o, non_corrected, Q); put(o, Tn, (size_t)Q * 16); put(o, Own, (size_t)Q * 3); put(o, pos, (size_t)P * 3); put(o, ref, P); put(o, normals, P);
    return write_out(outp, o);
}

static int run_spread(FILE *f, const char *outp) {
    int32_t hd[4];
    if (fread(hd, 4, 4, f) != 4) return 1;
    const int K = hd[0], P = hd[1], nchild = hd[2], norigins = hd[3];
    std::vector<float> Tcw, gba, pos, posg;
    std::vector<uint8_t> ingba, ptin, bad;
    std::vector<int32_t> coff, child, origins, refkf;
    if (!rd(f, Tcw, (size_t)K * 16) || !rd(f, gba, (size_t)K * 16) || !rd(f, ingba, K) || !rd(f, coff, K + 1) || !rd(f, child, nchild) || !rd(f, origins, norigins) ||
        !rd(f, pos, (size_t)P * 3) || !rd(f, posg, (size_t)P * 3) || !rd(f, ptin, P) || !rd(f, refkf, P) || !rd(f, bad, P)) return 1;
    orbr_spread_in_t in;
    in.K = K; in.Tcw16 = Tcw.data(); in.TcwGBA16 = gba.data(); in.kf_in_gba = ingba.data(); in.child_off = coff.data(); in.child = child.data();
    in.origins = origins.data(); in.n_origins = norigins; in.P = P; in.pos3 = pos.data(); in.posGBA3 = posg.data(); in.pt_in_gba = ptin.data();
    in.ref_kf = refkf.data(); in.bad = bad.data();
    McSpreadPlan gp;
    if (!mc_plan_spread(&in, gp)) { fprintf(stderr, "%s (at %lld: %lld)\n", gp.what, gp.at, gp.v); return 3; }
    gp.parent.push_back(-1); gp.order.push_back(-1); gp.reached.push_back(0); gp.marked.push_back(0);
    std::vector<float> pout((size_t)P * 3 + 1, -77.f);
    std::vector<int32_t> status(P + 1, -77);
    McTree G;
    G.Tcw = Tcw.data(); G.TcwGBA = gba.data(); G.parent = gp.parent.data(); G.order = gp.order.data();
    McSpread S;
    S.Tcw = Tcw.data(); S.TcwGBA = gba.data(); S.pos = pos.data(); S.posGBA = posg.data(); S.pt_in_gba = ptin.data(); S.bad = bad.data();
    S.reached = gp.reached.data(); S.marked = gp.marked.data(); S.ref_kf = refkf.data(); S.pos_out = pout.data(); S.status = status.data();
    blockIdx.x = 0;
    for (int l = 1; l <= gp.levels; l++) {   // one launch per level
        const int first = gp.first[l], n = gp.first[l + 1] - gp.first[l];
        MC_FOR(i, n) mc_tree(G, G.order[first + i]);
    }
    { MC_FOR(p, P) mc_spread(S, p); }
    std::vector<float> Tnew((size_t)K * 16 + 1);
    for (int k = 0; k < K; k++) memcpy(&Tnew[(size_t)k * 16], gp.reached[k] ? &gba[(size_t)k * 16] : &Tcw[(size_t)k * 16], 64);
    std::vector<int32_t> lev(1, gp.levels);
    std::vector<uint8_t> o;
    put(o, Tnew, (size_t)K * 16); put(o, gba, (size_t)K * 16); put(o, gp.marked, K); put(o, gp.reached, K); put(o, pout, (size_t)P * 3); put(o, status, P); put(o, lev, 1);
    return write_out(outp, o);
}

int main(int argc, char **argv) {
    if (argc != 4) { fprintf(stderr, "usage: mapcorrect_lockstep loop|spread IN OUT\n"); return 2; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) return 1;
    const int rc = !strcmp(argv[1], "loop") ? run_loop(f, argv[3]) : !strcmp(argv[1], "spread") ? run_spread(f, argv[3]) : 2;
    fclose(f);
    return rc;
}
