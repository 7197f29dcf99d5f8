// orbx_mapcorrect_dev.h — the device code of orbx_mapcorrect.hip that needs no HIP header: the bodies of the k_mc_* kernels, the two map-sized
// loops of LoopClosing (reference: src/LoopClosing.cc:444-525 and :685-746).  orbx_mapcorrect.hip wraps them in kernels;
// tests/cpp/mapcorrect_lockstep.cc compiles the same text for the host with ORBX_COVIS_HOST defined, one thread per workgroup
// (tests/cpp/hip_lockstep.h comes first, and the program supplies the built-ins that header lacks).
//
// Every float is one thread's own: a 4x4 product, a Sim3 product or a point's walk over its list in list order.  The one result that
// several threads decide together, a point's owner, is a minimum of integers: no order of arrival can change it.
#pragma once
#include "orbx_covis_dev.h"
#include "orbx_cvmath.h"
#include "orbx_g2omath.h"

#ifdef ORBX_COVIS_HOST
#define MC_THREADS 1
#else
#define MC_THREADS 256
#endif
#define MC_NO_OWNER 0x7FFFFFFF   // owner[p] of a point that no query's feature names; a position is below Q

// the strided index loop of every kernel here: element i of n by thread (blockIdx.x, threadIdx.x)
#define MC_FOR(i, n) for (int i = (int)(blockIdx.x * MC_THREADS + threadIdx.x); i < (n); i += (int)(gridDim.x * MC_THREADS))

// KeyFrame::SetPose (src/KeyFrame.cc:70-84, pinned in host/frame_shim.h): Ow = -Rwc * tcw, one gemm with alpha = -1
__device__ __forceinline__ void mc_center(const float *Tcw, float *Ow) {
    float Rwc[9];
    transpose33(Tcw, Rwc, 4);
    const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]};
    gemv3(Rwc, tcw, Ow, -1.0);
}
// ... and the Twc it leaves for GetPoseInverse(): [Rwc Ow; 0 0 0 1]
__device__ __forceinline__ void mc_pose_inverse(const float *Tcw, float *Twc) {
    float Rwc[9], Ow[3];
    transpose33(Tcw, Rwc, 4);
    const float tcw[3] = {Tcw[3], Tcw[7], Tcw[11]};
    gemv3(Rwc, tcw, Ow, -1.0);
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) Twc[r * 4 + c] = Rwc[r * 3 + c];
        Twc[r * 4 + 3] = Ow[r];
    }
    Twc[12] = 0.f; Twc[13] = 0.f; Twc[14] = 0.f; Twc[15] = 1.f;
}
// g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of a pose's top rows (sim3.h:64-67: Quaterniond(R), not normalised)
__device__ __forceinline__ orbg_sim3_t mc_sim3_of_pose(const float *T) {
    double R[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R[r * 3 + c] = (double)T[r * 4 + c];
    orbg_sim3_t S;
    quat_from_R(R, S.q);
    S.t[0] = (double)T[3]; S.t[1] = (double)T[7]; S.t[2] = (double)T[11];
    S.s = 1.0;
    return S;
}

// ---- k_mc_sim3: src/LoopClosing.cc:457-479 and :513-522 for one query.  corrected_inv is g2oCorrectedSwi (:486) for k_mc_points
struct McLoop { const float *Tiw; orbg_sim3_t Scw; int32_t Q, cur_pos; orbg_sim3_t *corrected, *non_corrected, *corrected_inv; float *Tiw_new, *Ow_new; };
__device__ __forceinline__ void mc_sim3(const McLoop &L, int q) {
    const float *Tiw = L.Tiw + (size_t)q * 16;
    orbg_sim3_t c = L.Scw;   // :449
    if (q != L.cur_pos) {
        float Twc[16], Tic[16];
        mc_pose_inverse(L.Tiw + (size_t)L.cur_pos * 16, Twc);   // :450
        gemm44(Tiw, Twc, Tic);                                  // :465
        c = sim3_mul(mc_sim3_of_pose(Tic), L.Scw);              // :468-469
    }
    L.corrected[q] = c;
    L.non_corrected[q] = mc_sim3_of_pose(Tiw);                  // :474-478
    L.corrected_inv[q] = sim3_inverse(c);
    double R[9];
    quat_to_R(c.q, R);                                          // :514
    const double k = 1. / c.s;                                  // :518: a multiply by the reciprocal
    float *T = L.Tiw_new + (size_t)q * 16;                      // Converter::toCvSE3
    for (int r = 0; r < 3; r++) {
        for (int j = 0; j < 3; j++) T[r * 4 + j] = (float)R[r * 3 + j];
        T[r * 4 + 3] = (float)(c.t[r] * k);
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
    mc_center(T, L.Ow_new + (size_t)q * 3);                     // :522
}

// ---- k_mc_owner: the query of the smallest position that names a point is the one whose loop corrects it (:491-499: the later ones
// meet mnCorrectedByKF).  One thread per feature of the concatenated lists; its query by bisection of feat_off
__device__ __forceinline__ void mc_owner(const CovTable &T, const CovQueries &Qs, int f, int32_t *owner) {
    int lo = 0, hi = Qs.Q;   // the q with feat_off[q] <= f < feat_off[q + 1]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (Qs.feat_off[mid] <= f) lo = mid; else hi = mid;
    }
    const int p = Qs.feat[f].point;
    if (p >= 0 && !T.pts[p].bad) atomicMin(&owner[p], lo);
}

// ---- k_mc_points: :501-510 for one point.  An observer's centre is the corrected one if it is a query at a position strictly below
// the owner's: those keyframes' SetPose (:522) ran before the owner's point loop, the owner's own comes after it
struct McPoints { const int32_t *qpos, *query_kf, *owner; const orbg_sim3_t *non_corrected, *corrected_inv; const float *Ow_new;
                  float *pos; int32_t *corrected_ref; orbc_normal_t *normals; };
__device__ __forceinline__ void mc_point(const CovTable &T, const McPoints &M, int p) {
    const int o = M.owner[p];
    const float *pin = T.pts[p].pos;
    float *pout = M.pos + (size_t)p * 3;
    if (o == MC_NO_OWNER) {
        pout[0] = pin[0]; pout[1] = pin[1]; pout[2] = pin[2];
        M.corrected_ref[p] = -1;
        orbc_normal_t r;
        r.normal[0] = 0.f; r.normal[1] = 0.f; r.normal[2] = 0.f; r.max_distance = 0.f; r.min_distance = 0.f; r.status = ORBR_NORMAL_UNTOUCHED;
        M.normals[p] = r;
        return;
    }
    const double P3Dw[3] = {(double)pin[0], (double)pin[1], (double)pin[2]};
    double mid[3], out[3];
    sim3_map(M.non_corrected[o], P3Dw, mid);    // :504
    sim3_map(M.corrected_inv[o], mid, out);
    const float np[3] = {(float)out[0], (float)out[1], (float)out[2]};   // Converter::toCvMat
    pout[0] = np[0]; pout[1] = np[1]; pout[2] = np[2];
    M.corrected_ref[p] = M.query_kf[o];         // :509
    M.normals[p] = cov_normal_at(T, p, np, [&T, &M, o](int k) -> const float * {
        const int qp = M.qpos[k];
        return qp >= 0 && qp < o ? M.Ow_new + (size_t)qp * 3 : T.kf[k].Ow;
    });
}

// ---- k_mc_tree: :696-701 for one keyframe outside the global BA whose parent's mTcwGBA is final (the host launches level by level).
// Twc is the parent's GetPoseInverse() before its SetPose(mTcwGBA) (:692 stands before :707): from its OLD pose
struct McTree { const float *Tcw; float *TcwGBA; const int32_t *parent, *order; };
__device__ __forceinline__ void mc_tree(const McTree &G, int c) {
    const int p = G.parent[c];
    float Twc[16], Tchildc[16], R[16];
    mc_pose_inverse(G.Tcw + (size_t)p * 16, Twc);
    gemm44(G.Tcw + (size_t)c * 16, Twc, Tchildc);      // :698
    gemm44(Tchildc, G.TcwGBA + (size_t)p * 16, R);     // :699
    for (int k = 0; k < 16; k++) G.TcwGBA[(size_t)c * 16 + k] = R[k];
}

// ---- k_mc_spread: :714-745 for one point; TcwGBA is final
struct McSpread { const float *Tcw, *TcwGBA, *pos, *posGBA; const uint8_t *pt_in_gba, *bad, *reached, *marked; const int32_t *ref_kf;
                  float *pos_out; int32_t *status; };
__device__ __forceinline__ void mc_spread(const McSpread &S, int p) {
    const float *pin = S.pos + (size_t)p * 3;
    float r[3] = {pin[0], pin[1], pin[2]};
    int st = ORBR_SPREAD_UNTOUCHED;
    if (!S.bad[p]) {   // :718
        const int k = S.ref_kf[p];
        if (S.pt_in_gba[p]) {   // :721-725
            r[0] = S.posGBA[(size_t)p * 3]; r[1] = S.posGBA[(size_t)p * 3 + 1]; r[2] = S.posGBA[(size_t)p * 3 + 2];
            st = ORBR_SPREAD_GBA;
        } else if (k < 0 || (S.marked[k] && !S.reached[k])) st = ORBR_SPREAD_UNDEFINED;   // a NULL reference keyframe, or an empty mTcwBefGBA
        else if (S.marked[k]) {   // :731
            const float *Tbef = S.Tcw + (size_t)k * 16, *Tnew = S.TcwGBA + (size_t)k * 16;
            const float tcw[3] = {Tbef[3], Tbef[7], Tbef[11]};
            float Xc[3], Rwc[9], twc[3];
            gemv3_add(Tbef, pin, tcw, Xc, 4);   // :735-737
            transpose33(Tnew, Rwc, 4);          // :740-742: the Twc SetPose derived from the new pose
            mc_center(Tnew, twc);
            gemv3_add(Rwc, Xc, twc, r);         // :744
            st = ORBR_SPREAD_MOVED;
        }
    }
    S.pos_out[(size_t)p * 3] = r[0]; S.pos_out[(size_t)p * 3 + 1] = r[1]; S.pos_out[(size_t)p * 3 + 2] = r[2];
    S.status[p] = st;
}
