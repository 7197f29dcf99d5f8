// orbx_newpoints.hip — the body of LocalMapping::CreateNewMapPoints (reference: src/LocalMapping.cc:215-460): what happens to the
// pairs ORBmatcher::SearchForTriangulation returns.  k_new_points is :299-439 statement by statement, one thread per match: the
// ray-parallax test, the 4x4 SVD (svd4_null of orbx_jacobi_svd.h, as Initializer::Triangulate runs it here) or
// KeyFrame::UnprojectStereo (src/KeyFrame.cc:618-634), two depth tests, two chi-square reprojection tests, the scale-consistency
// test.  cv::Mat expressions are evaluated as OpenCV evaluates them on CV_32F (orbx_cvmath.h); DESIGN.md section 6 has the list and
// tests/newpoints_ref.py is the same arithmetic in numpy.  The reference's oddities are kept, each with a comment naming its line.
//
// The matches of all keyframe pairs of a call share one grid: a workgroup serves ONE pair (NpBlock says which, and where in the
// pair's matches it starts), stages the pair's constants - the two views, the two level tables - in LDS once and forms the two Rwc
// and ratioFactor there.  A match's work is independent of every other: no sums across threads, no atomics, so two runs give the
// same bits.  Every byte of every output row is written here.
#ifdef ORBX_NEWPOINTS_HOST
// tests/cpp/newpoints_lockstep.cc compiles the kernel's text for the host as ONE thread per workgroup (tests/cpp/hip_lockstep.h comes
// first); of the host side the argument checks, orbl_baseline_ok and orbl_compute_f12 are compiled there.
#define NP_THREADS 1
#else
#include "orbx_stage.h"
#define NP_THREADS 256
#endif
#include <float.h>
#include <math.h>
#include "orbx_cvmath.h"
#include "orbx_jacobi_svd.h"

struct NpSide { orbl_view_t v; float sf[ORBL_MAX_LEVELS], sig2[ORBL_MAX_LEVELS]; int32_t kpOff, stOff, n, pad; };   // offsets in bytes from the scratch base; stOff < 0: a monocular keyframe
struct NpPair { NpSide s1, s2; int32_t off, n; };                                                                   // the pair's first output row and its number of rows
struct NpBlock { int32_t pair, first; };
struct NpFeat { float x, y; int32_t octave; float ur, depth, ru, rv; };

// :299-439 for one match.  P: the pair; Rwc1, Rwc2: the exact transposes of the views' Rcw
__device__ __forceinline__ orbl_point_t np_point(const NpPair &P, const float *Rwc1, const float *Rwc2, float ratioFactor, const NpFeat &f1, const NpFeat &f2) {
    const orbl_view_t &V1 = P.s1.v, &V2 = P.s2.v;
    orbl_point_t o;
    o.x = 0.f; o.y = 0.f; o.z = 0.f; o.status = 0; o.reserved[0] = 0; o.reserved[1] = 0;
    const bool bStereo1 = f1.ur >= 0, bStereo2 = f2.ur >= 0;   // :301, :305
    // Check parallax between rays (:308-313): xn in float, ray = Rwc * xn a cv::Mat product, the dot product a double
    const float xn1[3] = {(f1.x - V1.cx) * V1.invfx, (f1.y - V1.cy) * V1.invfy, 1.f};
    const float xn2[3] = {(f2.x - V2.cx) * V2.invfx, (f2.y - V2.cy) * V2.invfy, 1.f};
    float ray1[3], ray2[3];
    gemv3(Rwc1, xn1, ray1);
    gemv3(Rwc2, xn2, ray2);
    const double dot = ((double)ray1[0] * (double)ray2[0] + (double)ray1[1] * (double)ray2[1]) + (double)ray1[2] * (double)ray2[2];
    const float cosParallaxRays = (float)(dot / (norm3(ray1) * norm3(ray2)));
    float cosParallaxStereo = cosParallaxRays + 1;
    float cosParallaxStereo1 = cosParallaxStereo, cosParallaxStereo2 = cosParallaxStereo;
    // :319-322: `else if` - with both features stereo only keyframe 1's angle is formed.  <cmath>'s float overloads
    if (bStereo1) cosParallaxStereo1 = cosf(2 * atan2f(V1.mb / 2, f1.depth));
    else if (bStereo2) cosParallaxStereo2 = cosf(2 * atan2f(V2.mb / 2, f2.depth));
    cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min (:324)
    o.cos_rays = cosParallaxRays; o.cos_stereo = cosParallaxStereo;
    float x3D[3];
    int accepted;
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {   // :327, 0.9998 a double
        // Linear Triangulation Method (:330-345): the rows as written, in float
        float A[16], x[4];
        for (int c = 0; c < 4; c++) {
            A[c] = xn1[0] * V1.Tcw[8 + c] - V1.Tcw[c];
            A[4 + c] = xn1[1] * V1.Tcw[8 + c] - V1.Tcw[4 + c];
            A[8 + c] = xn2[0] * V2.Tcw[8 + c] - V2.Tcw[c];
            A[12 + c] = xn2[1] * V2.Tcw[8 + c] - V2.Tcw[4 + c];
        }
        svd4_null(A, x);
        if (x[3] == 0) { o.status = -2; return o; }   // :341
        x3D[0] = x[0] / x[3]; x3D[1] = x[1] / x[3]; x3D[2] = x[2] / x[3];
        accepted = 0;
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {   // :348, KeyFrame::UnprojectStereo: mvKeys (the RAW keypoint), not mvKeysUn
        const float z = f1.depth;
        const float xc[3] = {(f1.ru - V1.cx) * z * V1.invfx, (f1.rv - V1.cy) * z * V1.invfy, z};
        gemv3_add(Rwc1, xc, V1.Ow, x3D);
        accepted = 1;
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {   // :352
        const float z = f2.depth;
        const float xc[3] = {(f2.ru - V2.cx) * z * V2.invfx, (f2.rv - V2.cy) * z * V2.invfy, z};
        gemv3_add(Rwc2, xc, V2.Ow, x3D);
        accepted = 2;
    } else { o.status = -1; return o; }   // :357 No stereo and very low parallax
    o.x = x3D[0]; o.y = x3D[1]; o.z = x3D[2];
    // Check triangulation in front of cameras (:362-368)
    const float z1 = dot3_add(V1.Tcw + 8, x3D, V1.Tcw[11]);
    if (z1 <= 0) { o.status = -3; return o; }
    const float z2 = dot3_add(V2.Tcw + 8, x3D, V2.Tcw[11]);
    if (z2 <= 0) { o.status = -4; return o; }
    // Check reprojection error in first keyframe (:371-395)
    {
        const float sigmaSquare1 = P.s1.sig2[f1.octave];
        const float x1 = dot3_add(V1.Tcw, x3D, V1.Tcw[3]), y1 = dot3_add(V1.Tcw + 4, x3D, V1.Tcw[7]);
        const float invz1 = (float)(1.0 / (double)z1);
        const float u1 = V1.fx * x1 * invz1 + V1.cx, v1 = V1.fy * y1 * invz1 + V1.cy;
        const float errX1 = u1 - f1.x, errY1 = v1 - f1.y;
        if (!bStereo1) {
            if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigmaSquare1) { o.status = -5; return o; }
        } else {
            const float u1_r = u1 - V1.mbf * invz1;
            const float errX1_r = u1_r - f1.ur;
            if ((double)(errX1 * errX1 + errY1 * errY1 + errX1_r * errX1_r) > 7.8 * (double)sigmaSquare1) { o.status = -5; return o; }
        }
    }
    // Check reprojection error in second keyframe (:398-421)
    {
        const float sigmaSquare2 = P.s2.sig2[f2.octave];
        const float x2 = dot3_add(V2.Tcw, x3D, V2.Tcw[3]), y2 = dot3_add(V2.Tcw + 4, x3D, V2.Tcw[7]);
        const float invz2 = (float)(1.0 / (double)z2);
        const float u2 = V2.fx * x2 * invz2 + V2.cx, v2 = V2.fy * y2 * invz2 + V2.cy;
        const float errX2 = u2 - f2.x, errY2 = v2 - f2.y;
        if (!bStereo2) {
            if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigmaSquare2) { o.status = -6; return o; }
        } else {
            const float u2_r = u2 - V1.mbf * invz2;   // :414: mpCurrentKeyFrame->mbf, the FIRST keyframe's, for the second keyframe
            const float errX2_r = u2_r - f2.ur;
            if ((double)(errX2 * errX2 + errY2 * errY2 + errX2_r * errX2_r) > 7.8 * (double)sigmaSquare2) { o.status = -6; return o; }
        }
    }
    // Check scale consistency (:424-439)
    const float normal1[3] = {x3D[0] - V1.Ow[0], x3D[1] - V1.Ow[1], x3D[2] - V1.Ow[2]};
    const float normal2[3] = {x3D[0] - V2.Ow[0], x3D[1] - V2.Ow[1], x3D[2] - V2.Ow[2]};
    const float dist1 = (float)norm3(normal1), dist2 = (float)norm3(normal2);
    if (dist1 == 0 || dist2 == 0) { o.status = -7; return o; }
    const float ratioDist = dist2 / dist1;
    const float ratioOctave = P.s1.sf[f1.octave] / P.s2.sf[f2.octave];
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) { o.status = -8; return o; }   // :438, both sides
    o.status = accepted;
    return o;
}

__device__ __forceinline__ NpFeat np_feature(const NpSide &S, const uint8_t *base, int idx) {
    const orbx_keypoint_t *kp = (const orbx_keypoint_t *)(base + S.kpOff) + idx;
    NpFeat f;
    f.x = kp->x; f.y = kp->y; f.octave = kp->octave;
    f.ur = -1.f; f.depth = 0.f; f.ru = 0.f; f.rv = 0.f;
    if (S.stOff >= 0) {
        const orbl_stereo_t *st = (const orbl_stereo_t *)(base + S.stOff) + idx;
        f.ur = st->ur; f.depth = st->depth; f.ru = st->raw_u; f.rv = st->raw_v;
    }
    return f;
}

// matches != NULL: the pair's row r is (matches[2 r], matches[2 r + 1]).  matches == NULL (the chain form): one pair, row i is query
// feature i and match_q[i] its match; no match: status -10; an accepted row clears bit 0 of q_flags[i], so that the next
// neighbour's matcher no longer takes the feature as a query (src/ORBmatcher.cc:703-704 after :447)
__global__ __launch_bounds__(NP_THREADS) void k_new_points(const NpPair *__restrict__ pairs, const NpBlock *__restrict__ blocks, const uint8_t *__restrict__ base,
                                                           const int32_t *__restrict__ matches, const int32_t *__restrict__ match_q,
                                                           orbl_point_t *__restrict__ out, uint8_t *__restrict__ q_flags) {
    __shared__ NpPair P;
    __shared__ float Rwc[2][9];
    __shared__ float ratioFactor;
    const NpBlock b = blocks[blockIdx.x];
#ifdef ORBX_NEWPOINTS_HOST
    P = pairs[b.pair];
#else
    {
        const uint32_t *src = (const uint32_t *)(pairs + b.pair);
        uint32_t *dst = (uint32_t *)&P;
        for (int k = threadIdx.x; k < (int)(sizeof(NpPair) / 4); k += NP_THREADS) dst[k] = src[k];
    }
#endif
    __syncthreads();
    if (threadIdx.x == 0) {
        transpose33(P.s1.v.Tcw, Rwc[0], 4);             // Rwc = Rcw.t() (:226, :279)
        transpose33(P.s2.v.Tcw, Rwc[1], 4);
        ratioFactor = 1.5f * P.s1.v.scale_factor;       // :240
    }
    __syncthreads();
    const int i = b.first + (int)threadIdx.x;
    if (i >= P.n) return;
    const size_t row = (size_t)P.off + (size_t)i;
    int idx1, idx2;
    if (matches) { idx1 = matches[2 * row]; idx2 = matches[2 * row + 1]; }
    else { idx1 = i; idx2 = match_q[i]; }
    orbl_point_t o;
    if ((unsigned)idx1 >= (unsigned)P.s1.n || (unsigned)idx2 >= (unsigned)P.s2.n) {   // the host has checked a list of pairs; the chain form's -1
        o.x = 0.f; o.y = 0.f; o.z = 0.f; o.status = -10; o.cos_rays = 0.f; o.cos_stereo = 0.f; o.reserved[0] = 0; o.reserved[1] = 0;
    } else {
        o = np_point(P, Rwc[0], Rwc[1], ratioFactor, np_feature(P.s1, base, idx1), np_feature(P.s2, base, idx2));
        if (!matches && o.status >= 0) q_flags[idx1] = (uint8_t)(q_flags[idx1] & 0xFE);
    }
    out[row] = o;
}

// ------------------------------------------------------------------------------------
// host code: no device
static bool np_nan(const float *p, int n) {
    for (int k = 0; k < n; k++)
        if (p[k] != p[k]) return true;
    return false;
}
// the argument checks of one keyframe, before a device is touched (compiled for the host-only test program too)
static int np_check_keyframe(const char *fn, const orbl_keyframe_t *k) {
    if (!k || !k->view || k->n < 0 || !k->scale_factors || !k->level_sigma2 || (k->n > 0 && !k->kp)) { orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG; }
    const orbl_view_t &v = *k->view;
    if (v.nlevels < 1 || v.nlevels > ORBL_MAX_LEVELS) { orbx_set_error("%s: nlevels %d outside 1..%d", fn, v.nlevels, ORBL_MAX_LEVELS); return ORBX_ERR_ARG; }
    if (np_nan(v.Tcw, 16) || np_nan(v.Ow, 3) || np_nan(&v.fx, 9)) { orbx_set_error("%s: NaN in a view", fn); return ORBX_ERR_ARG; }
    for (int l = 0; l < v.nlevels; l++)
        if (!(k->level_sigma2[l] > 0.f) || !(k->scale_factors[l] > 0.f)) { orbx_set_error("%s: level %d: sigma2 or scale factor is not positive", fn, l); return ORBX_ERR_ARG; }
    for (int i = 0; i < k->n; i++) {
        const orbx_keypoint_t &p = k->kp[i];
        if (p.x != p.x || p.y != p.y) { orbx_set_error("%s: keypoint %d is NaN", fn, i); return ORBX_ERR_ARG; }
        if (p.octave < 0 || p.octave >= v.nlevels) { orbx_set_error("%s: keypoint %d: octave %d outside [0, %d)", fn, i, p.octave, v.nlevels); return ORBX_ERR_ARG; }
        if (k->st) {
            const orbl_stereo_t &s = k->st[i];
            if (np_nan(&s.ur, 4)) { orbx_set_error("%s: stereo feature %d is NaN", fn, i); return ORBX_ERR_ARG; }
            if (s.ur >= 0 && !(s.depth > 0.f)) { orbx_set_error("%s: stereo feature %d has depth <= 0", fn, i); return ORBX_ERR_ARG; }
        }
    }
    return ORBX_OK;
}
static int np_check_batch(const char *fn, const orbl_keyframe_t *kf1, const orbl_keyframe_t *kf2, int npairs, const int32_t *match_off, const int32_t *pairs,
                          orbl_point_t *points, int32_t *nnew) {
    if (npairs < 0 || !match_off || (npairs > 0 && (!kf1 || !kf2 || !nnew))) { orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG; }
    if (match_off[0] != 0) { orbx_set_error("%s: match_off[0] is not 0", fn); return ORBX_ERR_ARG; }
    for (int p = 0; p < npairs; p++)
        if (match_off[p + 1] < match_off[p]) { orbx_set_error("%s: match_off is not monotone", fn); return ORBX_ERR_ARG; }
    const int total = match_off[npairs];
    if (total > 0 && (!pairs || !points)) { orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG; }
    int rc = ORBX_OK;
    for (int p = 0; p < npairs && !rc; p++) {
        rc = np_check_keyframe(fn, kf1 + p);
        if (!rc) rc = np_check_keyframe(fn, kf2 + p);
        for (int r = match_off[p]; r < match_off[p + 1] && !rc; r++)
            if (pairs[2 * r] < 0 || pairs[2 * r] >= kf1[p].n || pairs[2 * r + 1] < 0 || pairs[2 * r + 1] >= kf2[p].n) {
                orbx_set_error("%s: match %d of pair %d is out of range", fn, r - match_off[p], p); rc = ORBX_ERR_ARG;
            }
    }
    if (rc) {   // the outputs are zeroed, as the other solvers do
        if (total > 0) memset(points, 0, (size_t)total * sizeof(orbl_point_t));
        for (int p = 0; p < npairs; p++) nnew[p] = 0;
    }
    return rc;
}

extern "C" int orbl_baseline_ok(const orbl_view_t *view1, const orbl_view_t *view2, int monocular, float median_depth2) {
    if (!view1 || !view2) { orbx_set_error("orbl_baseline_ok: bad arguments"); return ORBX_ERR_ARG; }
    const float vBaseline[3] = {view2->Ow[0] - view1->Ow[0], view2->Ow[1] - view1->Ow[1], view2->Ow[2] - view1->Ow[2]};   // :254
    const float baseline = (float)norm3(vBaseline);
    if (!monocular) return baseline < view2->mb ? 0 : 1;         // :259
    const float ratioBaselineDepth = baseline / median_depth2;   // :265
    return (double)ratioBaselineDepth < 0.01 ? 0 : 1;            // :267
}

extern "C" int orbl_compute_f12(const float *Tcw1_16, const float *K1_4, const float *Tcw2_16, const float *K2_4, float *F12_9) {
    if (!Tcw1_16 || !K1_4 || !Tcw2_16 || !K2_4 || !F12_9) { orbx_set_error("orbl_compute_f12: bad arguments"); return ORBX_ERR_ARG; }
    float R1w[9], R2w[9], t1w[3], t2w[3];
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { R1w[r * 3 + c] = Tcw1_16[r * 4 + c]; R2w[r * 3 + c] = Tcw2_16[r * 4 + c]; }
        t1w[r] = Tcw1_16[r * 4 + 3]; t2w[r] = Tcw2_16[r * 4 + 3];
    }
    float R12[9], mR12[9], t12[3];
    gemm33<true>(R1w, R2w, R12);          // R1w*R2w.t()                                   (:551)
    gemm33<true>(R1w, R2w, mR12, -1.0);   // -R1w*R2w.t(): a gemm with alpha -1, materialised (:552)
    gemv3_add(mR12, t2w, t1w, t12);       // ... *t2w+t1w: a gemm with an addend
    const float t12x[9] = {0.f, -t12[2], t12[1], t12[2], 0.f, -t12[0], -t12[1], t12[0], 0.f};   // SkewSymmetricMatrix (:706-711)
    const float K1t[9] = {K1_4[0], 0.f, 0.f, 0.f, K1_4[1], 0.f, K1_4[2], K1_4[3], 1.f};          // K1.t()
    const float K2[9] = {K2_4[0], 0.f, K2_4[2], 0.f, K2_4[1], K2_4[3], 0.f, 0.f, 1.f};
    float K1ti[9], K2i[9], a[9], b[9];
    invert33(K1t, K1ti);                  // K1.t().inv()
    invert33(K2, K2i);                    // K2.inv()
    gemm33(K1ti, t12x, a);                // ((K1.t().inv()*t12x)*R12)*K2.inv(), each product materialised (:560)
    gemm33(a, R12, b);
    gemm33(b, K2i, F12_9);
    return ORBX_OK;
}

#ifndef ORBX_NEWPOINTS_HOST
// host side: this thread's staging pair (orbx_stage.h)
static thread_local StagePair g_np;
void orbx_internal_release_newpoints_scratch() { g_np.release(); }

static void np_fill_side(NpSide &S, const orbl_keyframe_t &k, int32_t kpOff, int32_t stOff) {
    S.v = *k.view;
    for (int l = 0; l < ORBL_MAX_LEVELS; l++) { const int s = l < S.v.nlevels ? l : S.v.nlevels - 1; S.sf[l] = k.scale_factors[s]; S.sig2[l] = k.level_sigma2[s]; }
    S.kpOff = kpOff; S.stOff = stOff; S.n = k.n; S.pad = 0;
}

extern "C" int orbl_triangulate_batch(const orbl_keyframe_t *kf1, const orbl_keyframe_t *kf2, int npairs, const int32_t *match_off,
                                      const int32_t *pairs, orbl_point_t *points, int32_t *nnew, int device) {
    const int crc = np_check_batch("orbl_triangulate_batch", kf1, kf2, npairs, match_off, pairs, points, nnew);
    if (crc) return crc;
    for (int p = 0; p < npairs; p++) nnew[p] = 0;
    const int total = npairs > 0 ? match_off[npairs] : 0;
    if (total == 0) return ORBX_OK;
    int nblocks = 0;
    for (int p = 0; p < npairs; p++) nblocks += (match_off[p + 1] - match_off[p] + NP_THREADS - 1) / NP_THREADS;
    // upload block: pairs | blocks | matches | the keyframes' features (an array given twice, as the current keyframe of every pair is, goes up once);
    // download block: points
    StagePlan pl;
    const size_t oPair = pl.take((size_t)npairs * sizeof(NpPair)), oBlk = pl.take((size_t)nblocks * sizeof(NpBlock)), oM = pl.take((size_t)total * 8);
    struct Up { const void *src; size_t bytes, off; };
    std::vector<Up> ups;
    auto place = [&](const void *src, size_t bytes) -> size_t {
        for (const Up &u : ups)
            if (u.src == src && u.bytes == bytes) return u.off;
        ups.push_back({src, bytes, pl.take(bytes)});
        return ups.back().off;
    };
    std::vector<size_t> offs((size_t)npairs * 4, 0);
    for (int p = 0; p < npairs; p++) {
        if (match_off[p + 1] == match_off[p]) continue;
        offs[p * 4 + 0] = place(kf1[p].kp, (size_t)kf1[p].n * sizeof(orbx_keypoint_t));
        if (kf1[p].st) offs[p * 4 + 1] = place(kf1[p].st, (size_t)kf1[p].n * sizeof(orbl_stereo_t));
        offs[p * 4 + 2] = place(kf2[p].kp, (size_t)kf2[p].n * sizeof(orbx_keypoint_t));
        if (kf2[p].st) offs[p * 4 + 3] = place(kf2[p].st, (size_t)kf2[p].n * sizeof(orbl_stereo_t));
    }
    pl.mark_inputs();
    const size_t oOut = pl.take((size_t)total * sizeof(orbl_point_t));
    if (pl.off > (size_t)0x7FFFFFFF) { orbx_set_error("orbl_triangulate_batch: more than 2 GiB of staging"); return ORBX_ERR_UNSUPPORTED; }
    int rc = g_np.reserve(device, pl.off, (size_t)1 << 18);
    if (rc) return rc;
    uint8_t *d = g_np.d, *h = g_np.h;
    const hipStream_t st = g_np.stream;
    NpPair *hp = (NpPair *)(h + oPair);
    NpBlock *hb = (NpBlock *)(h + oBlk);
    int nb = 0;
    for (int p = 0; p < npairs; p++) {
        const int n = match_off[p + 1] - match_off[p];
        memset(&hp[p], 0, sizeof(NpPair));
        hp[p].off = match_off[p]; hp[p].n = n;
        if (n == 0) continue;   // no workgroup reads an empty pair's record
        np_fill_side(hp[p].s1, kf1[p], (int32_t)offs[p * 4 + 0], kf1[p].st ? (int32_t)offs[p * 4 + 1] : -1);
        np_fill_side(hp[p].s2, kf2[p], (int32_t)offs[p * 4 + 2], kf2[p].st ? (int32_t)offs[p * 4 + 3] : -1);
        for (int f = 0; f < n; f += NP_THREADS) { hb[nb].pair = p; hb[nb].first = f; nb++; }
    }
    memcpy(h + oM, pairs, (size_t)total * 8);
    for (const Up &u : ups) memcpy(h + u.off, u.src, u.bytes);
    ORBX_HIP(hipMemcpyAsync(d, h, pl.in_end, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_new_points, dim3(nblocks), dim3(NP_THREADS), 0, st, (const NpPair *)(d + oPair), (const NpBlock *)(d + oBlk), (const uint8_t *)d,
                       (const int32_t *)(d + oM), (const int32_t *)nullptr, (orbl_point_t *)(d + oOut), (uint8_t *)nullptr);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(h + oOut, d + oOut, (size_t)total * sizeof(orbl_point_t), hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    memcpy(points, h + oOut, (size_t)total * sizeof(orbl_point_t));
    for (int p = 0; p < npairs; p++)
        for (int r = match_off[p]; r < match_off[p + 1]; r++) nnew[p] += points[r].status >= 0;
    return ORBX_OK;
}

extern "C" int orbl_triangulate(const orbl_view_t *view1, const orbx_keypoint_t *kp1, const orbl_stereo_t *st1, int n1, const float *scale_factors1,
                                const float *level_sigma2_1, const orbl_view_t *view2, const orbx_keypoint_t *kp2, const orbl_stereo_t *st2, int n2,
                                const float *scale_factors2, const float *level_sigma2_2, const int32_t *pairs, int nm, orbl_point_t *points,
                                int *nnew, int device) {
    if (nm < 0 || !nnew) { orbx_set_error("orbl_triangulate: bad arguments"); return ORBX_ERR_ARG; }
    const orbl_keyframe_t k1 = {view1, kp1, st1, n1, scale_factors1, level_sigma2_1}, k2 = {view2, kp2, st2, n2, scale_factors2, level_sigma2_2};
    const int32_t off[2] = {0, nm};
    int32_t nn = 0;
    const int rc = orbl_triangulate_batch(&k1, &k2, 1, off, pairs, points, &nn, device);
    *nnew = nn;
    return rc;
}

// the chain's outputs as every error leaves them
static void np_chain_clean(int nq, int nn, const uint8_t *q_flags, int32_t *match_q, orbl_point_t *points, int32_t *nmatches, int32_t *nnew,
                           uint8_t *skipped, uint8_t *q_flags_out) {
    if (nn < 0 || nn > ORBL_MAX_NEIGHBOURS) nn = 0;
    if (nq > 0 && match_q) for (size_t i = 0; i < (size_t)nn * nq; i++) match_q[i] = -1;
    if (nq > 0 && points) memset(points, 0, (size_t)nn * nq * sizeof(orbl_point_t));
    for (int i = 0; i < nn; i++) { if (nmatches) nmatches[i] = 0; if (nnew) nnew[i] = 0; if (skipped) skipped[i] = 0; }
    if (nq > 0 && q_flags && q_flags_out) memcpy(q_flags_out, q_flags, nq);
}

extern "C" int orbl_create_new_map_points(const orbl_keyframe_t *cur, const uint8_t *q_desc, const uint8_t *q_flags, const orbl_neighbour_t *nb, int nn,
                                          int monocular, int max_dist, int check_orientation, int32_t *match_q, orbl_point_t *points,
                                          int32_t *nmatches, int32_t *nnew, uint8_t *skipped, uint8_t *q_flags_out, int device) {
    const char *fn = "orbl_create_new_map_points";
    const int nq = cur ? cur->n : 0;
    int rc = ORBX_OK;
    if (!cur || nn < 0 || (nn > 0 && (!nb || !nmatches || !nnew || !skipped)) || (nq > 0 && (!q_desc || !q_flags || !q_flags_out || (nn > 0 && (!match_q || !points))))) {
        orbx_set_error("%s: bad arguments", fn); rc = ORBX_ERR_ARG;
    }
    if (!rc && nn > ORBL_MAX_NEIGHBOURS) { orbx_set_error("%s: %d neighbours, at most %d", fn, nn, ORBL_MAX_NEIGHBOURS); rc = ORBX_ERR_UNSUPPORTED; }
    if (!rc) rc = np_check_keyframe(fn, cur);
    for (int i = 0; i < nn && !rc; i++) {
        const orbl_neighbour_t &b = nb[i];
        rc = np_check_keyframe(fn, &b.kf);
        if (!rc && (b.nnodes < 0 || (b.kf.n > 0 && (!b.c_desc || !b.c_flags)) || (b.nnodes > 0 && (!b.node_qstart || !b.node_cstart)))) {   // F12, the epipole and the median depth pass as they are, as they pass the matcher: a sideways neighbour has no finite epipole
            orbx_set_error("%s: neighbour %d: bad arguments", fn, i); rc = ORBX_ERR_ARG;
        }
        if (!rc && nq > 0 && b.kf.n > 0 && b.nnodes > 0) rc = orbx_internal_tri_check(fn, b.node_qstart, b.q_items, nq, b.node_cstart, b.c_items, b.kf.n, b.nnodes);
    }
    np_chain_clean(nq, nn, q_flags, match_q, points, nmatches, nnew, skipped, q_flags_out);
    if (rc) return rc;
    if (nq == 0 || nn == 0) return ORBX_OK;
    // what each neighbour does: 0 = the matcher and the triangulation run, 1 = skipped by the baseline rule, 2 = nothing to match against
    int what[ORBL_MAX_NEIGHBOURS], live = 0;
    for (int i = 0; i < nn; i++) {
        what[i] = !orbl_baseline_ok(cur->view, nb[i].kf.view, monocular, nb[i].median_depth2) ? 1 : (nb[i].kf.n == 0 || nb[i].nnodes == 0) ? 2 : 0;
        live += what[i] == 0;
    }
    const size_t rowBytes = (size_t)nq * sizeof(orbl_point_t);
    if (live) {
        const int nblocks = (nq + NP_THREADS - 1) / NP_THREADS;
        // upload block: pairs | blocks | the current keyframe | per live neighbour its features, descriptors, flags and node lists | q_flags;
        // download block, which starts at q_flags: q_flags | per live neighbour match_q, rows, the matcher's two words; device only: the angles
        StagePlan pl;
        struct Nb { size_t kp, st, cd, cf, nqs, qi, ncs, ci, mq, rows, out, ca; };
        Nb o[ORBL_MAX_NEIGHBOURS];
        const size_t oPair = pl.take((size_t)nn * sizeof(NpPair)), oBlk = pl.take((size_t)nblocks * sizeof(NpBlock));
        const size_t oKp1 = pl.take((size_t)nq * sizeof(orbx_keypoint_t)), oSt1 = cur->st ? pl.take((size_t)nq * sizeof(orbl_stereo_t)) : 0, oQd = pl.take((size_t)nq * 32);
        for (int i = 0; i < nn; i++) {
            if (what[i]) continue;
            const orbl_neighbour_t &b = nb[i];
            const int nc = b.kf.n, tq = b.node_qstart[b.nnodes], tc = b.node_cstart[b.nnodes];
            o[i].kp = pl.take((size_t)nc * sizeof(orbx_keypoint_t)); o[i].st = b.kf.st ? pl.take((size_t)nc * sizeof(orbl_stereo_t)) : 0;
            o[i].cd = pl.take((size_t)nc * 32); o[i].cf = pl.take(nc);
            o[i].nqs = pl.take((size_t)(b.nnodes + 1) * 4); o[i].ncs = pl.take((size_t)(b.nnodes + 1) * 4);
            o[i].qi = pl.take((size_t)(tq > 0 ? tq : 1) * 4); o[i].ci = pl.take((size_t)(tc > 0 ? tc : 1) * 4);
        }
        const size_t oQf = pl.take(nq);
        pl.mark_inputs();
        for (int i = 0; i < nn; i++) {
            if (what[i]) continue;
            o[i].mq = pl.take((size_t)nq * 4); o[i].rows = pl.take(rowBytes); o[i].out = pl.take(16);
        }
        const size_t oEnd = pl.off, oQa = pl.take((size_t)nq * 4);
        for (int i = 0; i < nn; i++)
            if (!what[i]) o[i].ca = pl.take((size_t)nb[i].kf.n * 4);
        if (pl.off > (size_t)0x7FFFFFFF) { orbx_set_error("%s: more than 2 GiB of staging", fn); return ORBX_ERR_UNSUPPORTED; }
        rc = g_np.reserve(device, pl.off, (size_t)1 << 18);
        if (rc) return rc;
        uint8_t *d = g_np.d, *h = g_np.h;
        const hipStream_t st = g_np.stream;
        NpPair *hp = (NpPair *)(h + oPair);
        NpBlock *hb = (NpBlock *)(h + oBlk);
        for (int k = 0; k < nblocks; k++) { hb[k].pair = 0; hb[k].first = k * NP_THREADS; }
        memcpy(h + oKp1, cur->kp, (size_t)nq * sizeof(orbx_keypoint_t));
        if (cur->st) memcpy(h + oSt1, cur->st, (size_t)nq * sizeof(orbl_stereo_t));
        memcpy(h + oQd, q_desc, (size_t)nq * 32);
        memcpy(h + oQf, q_flags, nq);
        for (int i = 0; i < nn; i++) {
            memset(&hp[i], 0, sizeof(NpPair));
            if (what[i]) continue;
            const orbl_neighbour_t &b = nb[i];
            const int nc = b.kf.n, tq = b.node_qstart[b.nnodes], tc = b.node_cstart[b.nnodes];
            np_fill_side(hp[i].s1, *cur, (int32_t)oKp1, cur->st ? (int32_t)oSt1 : -1);
            np_fill_side(hp[i].s2, b.kf, (int32_t)o[i].kp, b.kf.st ? (int32_t)o[i].st : -1);
            hp[i].off = 0; hp[i].n = nq;
            memcpy(h + o[i].kp, b.kf.kp, (size_t)nc * sizeof(orbx_keypoint_t));
            if (b.kf.st) memcpy(h + o[i].st, b.kf.st, (size_t)nc * sizeof(orbl_stereo_t));
            memcpy(h + o[i].cd, b.c_desc, (size_t)nc * 32); memcpy(h + o[i].cf, b.c_flags, nc);
            memcpy(h + o[i].nqs, b.node_qstart, (size_t)(b.nnodes + 1) * 4); memcpy(h + o[i].ncs, b.node_cstart, (size_t)(b.nnodes + 1) * 4);
            if (tq > 0) memcpy(h + o[i].qi, b.q_items, (size_t)tq * 4);
            if (tc > 0) memcpy(h + o[i].ci, b.c_items, (size_t)tc * 4);
        }
        ORBX_HIP(hipMemcpyAsync(d, h, pl.in_end, hipMemcpyHostToDevice, st));
        (void)hipGetLastError();
        for (int i = 0; i < nn; i++) {
            if (what[i]) continue;
            const orbl_neighbour_t &b = nb[i];
            ORBX_HIP(hipMemsetAsync(d + o[i].mq, 0xFF, (size_t)nq * 4, st));
            ORBX_HIP(hipMemsetAsync(d + o[i].out, 0, 16, st));
            orbx_internal_tri_launch((const orbx_keypoint_t *)(d + oKp1), d + oQd, d + oQf, (float *)(d + oQa), nq, (const orbx_keypoint_t *)(d + o[i].kp), d + o[i].cd,
                                     d + o[i].cf, (float *)(d + o[i].ca), b.kf.n, (const int32_t *)(d + o[i].nqs), (const int32_t *)(d + o[i].qi),
                                     (const int32_t *)(d + o[i].ncs), (const int32_t *)(d + o[i].ci), b.nnodes, b.F12, b.ex, b.ey, b.kf.scale_factors,
                                     b.kf.level_sigma2, b.kf.view->nlevels, max_dist, check_orientation, (int32_t *)(d + o[i].mq), (int32_t *)(d + o[i].out), st);
            hipLaunchKernelGGL(k_new_points, dim3(nblocks), dim3(NP_THREADS), 0, st, (const NpPair *)(d + oPair) + i, (const NpBlock *)(d + oBlk), (const uint8_t *)d,
                               (const int32_t *)nullptr, (const int32_t *)(d + o[i].mq), (orbl_point_t *)(d + o[i].rows), d + oQf);
        }
        ORBX_HIP(hipGetLastError());
        ORBX_HIP(hipMemcpyAsync(h + oQf, d + oQf, oEnd - oQf, hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipStreamSynchronize(st));
        for (int i = 0; i < nn; i++)
            if (!what[i] && ((const int32_t *)(h + o[i].out))[1]) {
                orbx_set_error("%s: neighbour %d: a vocabulary node holds more than 4096 candidate features", fn, i);
                return ORBX_ERR_UNSUPPORTED;   // the outputs are as np_chain_clean left them
            }
        memcpy(q_flags_out, h + oQf, nq);
        for (int i = 0; i < nn; i++) {
            if (what[i]) continue;
            memcpy(match_q + (size_t)i * nq, h + o[i].mq, (size_t)nq * 4);
            memcpy(points + (size_t)i * nq, h + o[i].rows, rowBytes);
            nmatches[i] = ((const int32_t *)(h + o[i].out))[0];
            for (int r = 0; r < nq; r++) nnew[i] += points[(size_t)i * nq + r].status >= 0;
        }
    }
    for (int i = 0; i < nn; i++) {
        if (!what[i]) continue;
        skipped[i] = what[i] == 1;
        for (int r = 0; r < nq; r++) points[(size_t)i * nq + r].status = what[i] == 1 ? -9 : -10;
    }
    return ORBX_OK;
}
#endif   // ORBX_NEWPOINTS_HOST
