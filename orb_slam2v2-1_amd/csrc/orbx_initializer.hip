// orbx_initializer.hip — Initializer::Initialize (reference: src/Initializer.cc:44-929) as a chain of four launches on one stream:
//   k_init_normalize    Normalize over ALL keys of each frame (:749-795): T1, T2, T2inv, T2t                      2 workgroups
//   k_init_ransac       one hypothesis per workgroup of one wave: ComputeH21 / ComputeF21, CheckHomography /      2 x iterations
//                       CheckFundamental over all N matches (:226-468)
//   k_init_select       first strictly greater score per kind (:165, :216), RH, the choice (:112-118)             1 workgroup
//   k_init_reconstruct  ReconstructH / ReconstructF, CheckRT for every motion over every inlier, acceptance        1 workgroup
//                       (:470-732, :798-929)
// Float where the reference is CV_32F, double where it writes a double literal into a float expression, cv::gemm / cv::invert /
// cv::norm / cv::determinant are csrc/orbx_cvmath.h; the SVDs are csrc/orbx_jacobi_svd.h.  DESIGN.md section 6 has the list;
// tests/init_ref.py is the same arithmetic in numpy.  Sums whose order matters (the Normalize means, a hypothesis' score) are
// accumulated by ONE thread in the reference's order from terms the others computed in parallel: the bytes do not depend on
// the launch shape.  Every loop has a bound that is a constant or an argument.
#ifdef ORBX_INIT_HOST
// tests/cpp/initializer_lockstep.cc compiles the kernels' text for the host as ONE thread per workgroup (tests/cpp/hip_lockstep.h
// comes first) and runs the workgroups one after the other.  Nothing below the kernels is compiled there.
#define INI_RT 1
#define INI_BT 1
#else
#include "orbx_stage.h"
#define INI_RT 64     // k_init_ransac: one wave
#define INI_BT 256
#endif
#include <float.h>
#include <math.h>
#include "orbx_cvmath.h"
#include "orbx_jacobi_svd.h"

#define INI_CHUNK 512          // matches (k_init_ransac) or keys (k_init_normalize, x 2) whose terms are staged in LDS per ordered pass
#define INI_PI 3.1415926535897932384626433832795   // CV_PI

struct InitNorm { float T1[9], T2[9], T2inv[9], T2t[9]; float mean[4], scale[4]; };   // mean / scale: x1 y1 x2 y2
// keys: x at k[i * stride], y at k[i * stride + 1] (stride 2: packed pairs, 7: orbx_keypoint_t records)
struct InitIn {
    const float *k1, *k2; int s1, s2, n1, n2;
    const int32_t *matches; int N; const int32_t *sets; int iters;
    float sigma, fx, fy, cx, cy, minParallax; int minTri;
};
struct InitOut { int32_t result; float R[9], t[3]; };

// ---- Normalize (:749-795): workgroup 0 the reference frame, 1 the current one.  The four float sums are accumulated by thread 0
// in ascending key order from LDS; the others only stage the keys.
__global__ __launch_bounds__(INI_BT) void k_init_normalize(InitIn in, InitNorm *__restrict__ norm) {
    __shared__ float st[2 * INI_CHUNK * 2];
    __shared__ float mean[2];
    const int tid = threadIdx.x, f = blockIdx.x;
    const float *k = f ? in.k2 : in.k1;
    const int s = f ? in.s2 : in.s1, n = f ? in.n2 : in.n1;
    float meanX = 0, meanY = 0;
    for (int base = 0; base < n; base += 2 * INI_CHUNK) {
        const int cnt = n - base < 2 * INI_CHUNK ? n - base : 2 * INI_CHUNK;
        for (int j = tid; j < cnt; j += INI_BT) { st[2 * j] = k[(size_t)(base + j) * s]; st[2 * j + 1] = k[(size_t)(base + j) * s + 1]; }
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < cnt; j++) { meanX += st[2 * j]; meanY += st[2 * j + 1]; }
        __syncthreads();
    }
    if (tid == 0) { mean[0] = meanX / n; mean[1] = meanY / n; }
    __syncthreads();
    meanX = mean[0]; meanY = mean[1];
    float meanDevX = 0, meanDevY = 0;
    for (int base = 0; base < n; base += 2 * INI_CHUNK) {
        const int cnt = n - base < 2 * INI_CHUNK ? n - base : 2 * INI_CHUNK;
        for (int j = tid; j < cnt; j += INI_BT) {
            st[2 * j] = fabsf(k[(size_t)(base + j) * s] - meanX);
            st[2 * j + 1] = fabsf(k[(size_t)(base + j) * s + 1] - meanY);
        }
        __syncthreads();
        if (tid == 0)
            for (int j = 0; j < cnt; j++) { meanDevX += st[2 * j]; meanDevY += st[2 * j + 1]; }
        __syncthreads();
    }
    if (tid == 0) {
        meanDevX = meanDevX / n; meanDevY = meanDevY / n;
        const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
        float T[9] = {sX, 0.f, -meanX * sX, 0.f, sY, -meanY * sY, 0.f, 0.f, 1.f};
        norm->mean[2 * f] = meanX; norm->mean[2 * f + 1] = meanY; norm->scale[2 * f] = sX; norm->scale[2 * f + 1] = sY;
        if (f == 0) { for (int i = 0; i < 9; i++) norm->T1[i] = T[i]; }
        else {
            float Ti[9];
            invert33(T, Ti);
            for (int i = 0; i < 9; i++) { norm->T2[i] = T[i]; norm->T2inv[i] = Ti[i]; norm->T2t[i] = T[(i % 3) * 3 + i / 3]; }
        }
    }
}

// ---- one RANSAC hypothesis per workgroup: blocks 0..iters-1 the homographies, iters..2 iters-1 the fundamental matrices
__global__ __launch_bounds__(INI_RT) void k_init_ransac(InitIn in, const InitNorm *__restrict__ norm, float *__restrict__ models,
                                                       float *__restrict__ scores, uint8_t *__restrict__ inl) {
    __shared__ float W[25 * 9];              // 16 rows of A (the 8 of F zero-padded), 9 of V
    __shared__ float terms[2 * INI_CHUNK];
    const int tid = threadIdx.x, hyp = blockIdx.x, kind = hyp >= in.iters ? 1 : 0, it = kind ? hyp - in.iters : hyp, N = in.N;
    const InitNorm nm = *norm;
    for (int k = tid; k < 25 * 9; k += INI_RT) W[k] = (k >= 16 * 9 && (k - 16 * 9) / 9 == (k - 16 * 9) % 9) ? 1.f : 0.f;
    __syncthreads();
    for (int j = tid; j < 8; j += INI_RT) {
        const int idx = in.sets[it * 8 + j], m1 = in.matches[2 * idx], m2 = in.matches[2 * idx + 1];
        const float u1 = (in.k1[(size_t)m1 * in.s1] - nm.mean[0]) * nm.scale[0], v1 = (in.k1[(size_t)m1 * in.s1 + 1] - nm.mean[1]) * nm.scale[1];
        const float u2 = (in.k2[(size_t)m2 * in.s2] - nm.mean[2]) * nm.scale[2], v2 = (in.k2[(size_t)m2 * in.s2 + 1] - nm.mean[3]) * nm.scale[3];
        if (kind == 0) {   // ComputeH21 (:239-257)
            float *r0 = W + (2 * j) * 9, *r1 = r0 + 9;
            r0[0] = 0.f; r0[1] = 0.f; r0[2] = 0.f; r0[3] = -u1; r0[4] = -v1; r0[5] = -1.f; r0[6] = v2 * u1; r0[7] = v2 * v1; r0[8] = v2;
            r1[0] = u1; r1[1] = v1; r1[2] = 1.f; r1[3] = 0.f; r1[4] = 0.f; r1[5] = 0.f; r1[6] = -u2 * u1; r1[7] = -u2 * v1; r1[8] = -u2;
        } else {           // ComputeF21 (:281-289)
            float *r = W + j * 9;
            r[0] = u2 * u1; r[1] = u2 * v1; r[2] = u2; r[3] = v2 * u1; r[4] = v2 * v1; r[5] = v2; r[6] = u1; r[7] = v1; r[8] = 1.f;
        }
    }
    __syncthreads();
    jacobi_sweeps<16, 9, true>(W, tid, INI_RT);
    float w9[9], Mn[9], M21[9], M12[9], tmp[9];
    int order[9];
    jacobi_order<16, 9>(W, w9, order);
    for (int k = 0; k < 9; k++) Mn[k] = W[(16 + k) * 9 + order[8]];   // vt.row(8).reshape(0, 3)
    if (kind == 0) {
        gemm33(nm.T2inv, Mn, tmp); gemm33(tmp, nm.T1, M21);           // H21i = T2inv*Hn*T1
        invert33(M21, M12);                                           // H12i = H21i.inv()
    } else {
        float wf[3], U[9], Vt[9], D[9], Fn[9];
        svd3(Mn, wf, U, Vt);
        for (int k = 0; k < 9; k++) D[k] = 0.f;
        D[0] = wf[0]; D[4] = wf[1];                                   // w.at<float>(2) = 0
        gemm33(U, D, tmp); gemm33(tmp, Vt, Fn);                       // u*diag(w)*vt
        gemm33(nm.T2t, Fn, tmp); gemm33(tmp, nm.T1, M21);             // F21i = T2t*Fn*T1
        for (int k = 0; k < 9; k++) M12[k] = 0.f;
    }
    if (tid == 0)
        for (int k = 0; k < 9; k++) models[(size_t)hyp * 9 + k] = M21[k];

    const float invSigmaSquare = (float)(1.0 / (double)(in.sigma * in.sigma));
    const float thH = 5.991f, thF = 3.841f, thScore = 5.991f;
    float score = 0.f;
    uint8_t *flags = inl + (size_t)hyp * N;
    for (int base = 0; base < N; base += INI_CHUNK) {
        const int cnt = N - base < INI_CHUNK ? N - base : INI_CHUNK;
        for (int j = tid; j < cnt; j += INI_RT) {
            const int i = base + j, m1 = in.matches[2 * i], m2 = in.matches[2 * i + 1];
            const float u1 = in.k1[(size_t)m1 * in.s1], v1 = in.k1[(size_t)m1 * in.s1 + 1];
            const float u2 = in.k2[(size_t)m2 * in.s2], v2 = in.k2[(size_t)m2 * in.s2 + 1];
            bool bIn = true;
            float t1, t2;
            if (kind == 0) {   // CheckHomography (:337-385)
                const float w2in1inv = (float)(1.0 / (double)(M12[6] * u2 + M12[7] * v2 + M12[8]));
                const float u2in1 = (M12[0] * u2 + M12[1] * v2 + M12[2]) * w2in1inv;
                const float v2in1 = (M12[3] * u2 + M12[4] * v2 + M12[5]) * w2in1inv;
                const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
                const float chiSquare1 = squareDist1 * invSigmaSquare;
                if (chiSquare1 > thH) { bIn = false; t1 = 0.f; } else t1 = thH - chiSquare1;
                const float w1in2inv = (float)(1.0 / (double)(M21[6] * u1 + M21[7] * v1 + M21[8]));
                const float u1in2 = (M21[0] * u1 + M21[1] * v1 + M21[2]) * w1in2inv;
                const float v1in2 = (M21[3] * u1 + M21[4] * v1 + M21[5]) * w1in2inv;
                const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
                const float chiSquare2 = squareDist2 * invSigmaSquare;
                if (chiSquare2 > thH) { bIn = false; t2 = 0.f; } else t2 = thH - chiSquare2;
            } else {           // CheckFundamental (:413-465)
                const float a2 = M21[0] * u1 + M21[1] * v1 + M21[2];
                const float b2 = M21[3] * u1 + M21[4] * v1 + M21[5];
                const float c2 = M21[6] * u1 + M21[7] * v1 + M21[8];
                const float num2 = a2 * u2 + b2 * v2 + c2;
                const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
                const float chiSquare1 = squareDist1 * invSigmaSquare;
                if (chiSquare1 > thF) { bIn = false; t1 = 0.f; } else t1 = thScore - chiSquare1;
                const float a1 = M21[0] * u2 + M21[3] * v2 + M21[6];
                const float b1 = M21[1] * u2 + M21[4] * v2 + M21[7];
                const float c1 = M21[2] * u2 + M21[5] * v2 + M21[8];
                const float num1 = a1 * u1 + b1 * v1 + c1;
                const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
                const float chiSquare2 = squareDist2 * invSigmaSquare;
                if (chiSquare2 > thF) { bIn = false; t2 = 0.f; } else t2 = thScore - chiSquare2;
            }
            terms[2 * j] = t1; terms[2 * j + 1] = t2;
            flags[i] = bIn ? 1 : 0;
        }
        __syncthreads();
        if (tid == 0)
            for (int k = 0; k < 2 * cnt; k++) score += terms[k];   // the reference's order: match ascending, first image's term first
        __syncthreads();
    }
    if (tid == 0) scores[hyp] = score;
}

// ---- the two searches' winners (:165-170, :216-221), RH and the choice (:112-118)
__global__ __launch_bounds__(INI_BT) void k_init_select(InitIn in, const float *__restrict__ models, const float *__restrict__ scores,
                                                       const uint8_t *__restrict__ inl, uint8_t *__restrict__ inlBest,
                                                       orbi_init_info_t *__restrict__ info) {
    __shared__ int best[2], cnt[2];
    const int tid = threadIdx.x, N = in.N;
    for (int kind = tid; kind < 2; kind += INI_BT) {   // thread 0 the homographies, thread 1 the fundamental matrices
        float sc = 0.f;
        int bi = -1;
        for (int it = 0; it < in.iters; it++) {
            const float c = scores[kind * in.iters + it];
            if (c > sc) { sc = c; bi = it; }
        }
        best[kind] = bi; cnt[kind] = 0;
        if (kind == 0) info->SH = sc; else info->SF = sc;
        info->best_iteration[kind] = bi;
        float *M = kind == 0 ? info->H21 : info->F21;
        for (int k = 0; k < 9; k++) M[k] = bi < 0 ? 0.f : models[((size_t)kind * in.iters + bi) * 9 + k];
    }
    __syncthreads();
    for (int kind = 0; kind < 2; kind++) {
        const int bi = best[kind];
        int mine = 0;
        for (int i = tid; i < N; i += INI_BT) {
            const uint8_t f = bi < 0 ? 0 : inl[((size_t)kind * in.iters + bi) * N + i];
            inlBest[(size_t)kind * N + i] = f;
            mine += f;
        }
        if (mine) atomicAdd(&cnt[kind], mine);
    }
    __syncthreads();
    if (tid == 0) {
        const float SH = info->SH, SF = info->SF, RH = SH / (SH + SF);
        info->RH = RH;
        info->model = RH > 0.40f ? 0 : 1;     // a NaN ratio (both scores 0) takes the fundamental branch, as the reference's else does
        info->inliers[0] = cnt[0]; info->inliers[1] = cnt[1];
        info->best_good = 0; info->second_good = 0; info->parallax = 0.f; info->ncand = 0;
        for (int c = 0; c < 8; c++) { info->ngood[c] = 0; info->cand_parallax[c] = 0.f; }
    }
}

__device__ __forceinline__ uint32_t float_key(float f) {   // ascending floats -> ascending keys
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key_float(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// ---- ReconstructH / ReconstructF with CheckRT.  Every thread decomposes the model itself (uniform control flow, no broadcast);
// the matches of a motion are shared out, match i to thread i % 256.
__global__ __launch_bounds__(INI_BT) void k_init_reconstruct(InitIn in, const uint8_t *__restrict__ inlBest, float *__restrict__ candP,
                                                            uint8_t *__restrict__ candF, float *__restrict__ candC,
                                                            orbi_init_info_t *__restrict__ info, InitOut *__restrict__ out,
                                                            float *__restrict__ P3D, uint8_t *__restrict__ tri) {
    __shared__ int s_cnt[2];
    __shared__ int s_good[8];
    __shared__ float s_par[8];
    const int tid = threadIdx.x, N = in.N;
    const int model = info->model;
    const uint8_t *inlv = inlBest + (size_t)model * N;
    const int nInl = info->inliers[model];
    const float K[9] = {in.fx, 0.f, in.cx, 0.f, in.fy, in.cy, 0.f, 0.f, 1.f};
    float Rc[8][9], tc[8][3];
    int ncand = 0;
    if (info->best_iteration[model] >= 0) {
        if (model == 0) {   // ReconstructH (:584-686)
            float invK[9], tmp[9], A[9], w[3], U[9], Vt[9], V[9];
            invert33(K, invK);
            gemm33(invK, info->H21, tmp); gemm33(tmp, K, A);
            svd3(A, w, U, Vt);
            for (int k = 0; k < 9; k++) V[k] = Vt[(k % 3) * 3 + k / 3];
            const float s = (float)(det3(U) * det3(Vt));
            const float d1 = w[0], d2 = w[1], d3 = w[2];
            if (!((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001)) {
                ncand = 8;
                const float aux1 = sqrtf((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
                const float aux3 = sqrtf((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
                const float x1[4] = {aux1, aux1, -aux1, -aux1}, x3[4] = {aux3, -aux3, aux3, -aux3};
                const float aux_stheta = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
                const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
                const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
                const float aux_sphi = sqrtf((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
                const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
                const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
                for (int i = 0; i < 8; i++) {
                    const int j = i & 3;
                    float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3], t[3];
                    if (i < 4) { Rp[0] = ctheta; Rp[2] = -stheta[j]; Rp[6] = stheta[j]; Rp[8] = ctheta; }
                    else { Rp[0] = cphi; Rp[2] = sphi[j]; Rp[4] = -1.f; Rp[6] = sphi[j]; Rp[8] = -cphi; }
                    gemm33(U, Rp, tmp, (double)s); gemm33(tmp, Vt, Rc[i]);            // s*U*Rp*Vt
                    tp[0] = x1[j]; tp[1] = 0.f; tp[2] = i < 4 ? -x3[j] : x3[j];
                    const float dd = i < 4 ? d1 - d3 : d1 + d3;
                    tp[0] *= dd; tp[1] *= dd; tp[2] *= dd;
                    gemv3(U, tp, t);
                    const double inv = 1. / norm3(t);                                  // t / cv::norm(t)
                    for (int k = 0; k < 3; k++) tc[i][k] = (float)((double)t[k] * inv);
                }
                (void)V;   // the plane normals vn (V*np) feed nothing
            }
        } else {            // ReconstructF (:479-487), DecomposeE (:909-929)
            float Kt[9], tmp[9], E[9], w[3], U[9], Vt[9], t[3], R1[9], R2[9];
            for (int k = 0; k < 9; k++) Kt[k] = K[(k % 3) * 3 + k / 3];
            gemm33(Kt, info->F21, tmp); gemm33(tmp, K, E);
            svd3(E, w, U, Vt);
            t[0] = U[2]; t[1] = U[5]; t[2] = U[8];
            const double inv = 1. / norm3(t);
            for (int k = 0; k < 3; k++) t[k] = (float)((double)t[k] * inv);
            const float Wm[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Wt[9] = {0.f, 1.f, 0.f, -1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
            gemm33(U, Wm, tmp); gemm33(tmp, Vt, R1);
            if (det3(R1) < 0) for (int k = 0; k < 9; k++) R1[k] = -R1[k];
            gemm33(U, Wt, tmp); gemm33(tmp, Vt, R2);
            if (det3(R2) < 0) for (int k = 0; k < 9; k++) R2[k] = -R2[k];
            ncand = 4;
            for (int c = 0; c < 4; c++) {   // (R1, t) (R2, t) (R1, -t) (R2, -t)
                for (int k = 0; k < 9; k++) Rc[c][k] = (c & 1) ? R2[k] : R1[k];
                for (int k = 0; k < 3; k++) tc[c][k] = c < 2 ? t[k] : -t[k];
            }
        }
    }

    const float th2 = (float)(4.0 * (double)(in.sigma * in.sigma));   // 4.0*mSigma2
    for (int c = 0; c < ncand; c++) {   // CheckRT (:798-907)
        const float *R = Rc[c], *t = tc[c];
        float P2[12], O2[3], Rt[9];
        // P2 = K*[R|t] and R*p3dC1+t below are cv::gemm as in orbx_cvmath.h (the latter with its addend, + t in double), inline: a call of
        // N = 2000 matches is 12 us slower with them in helpers (profiles/README.md, the per-call figures of the shared staging pair)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 4; j++) {
                const float b0 = j < 3 ? R[j] : t[0], b1 = j < 3 ? R[3 + j] : t[1], b2 = j < 3 ? R[6 + j] : t[2];
                P2[i * 4 + j] = (float)(((double)K[i * 3] * (double)b0 + (double)K[i * 3 + 1] * (double)b1) + (double)K[i * 3 + 2] * (double)b2);
            }
        for (int k = 0; k < 9; k++) Rt[k] = R[(k % 3) * 3 + k / 3];
        gemv3(Rt, t, O2, -1.0);             // O2 = -R.t()*t
        if (tid == 0) s_cnt[0] = 0;
        __syncthreads();
        float *cp = candP + (size_t)c * N * 3, *cc = candC + (size_t)c * N;
        uint8_t *cf = candF + (size_t)c * N;
        int mine = 0;
        for (int i = tid; i < N; i += INI_BT) {
            cp[3 * i] = 0.f; cp[3 * i + 1] = 0.f; cp[3 * i + 2] = 0.f; cf[i] = 0; cc[i] = 0.f;
            if (!inlv[i]) continue;
            const int m1 = in.matches[2 * i], m2 = in.matches[2 * i + 1];
            const float x1 = in.k1[(size_t)m1 * in.s1], y1 = in.k1[(size_t)m1 * in.s1 + 1];
            const float x2 = in.k2[(size_t)m2 * in.s2], y2 = in.k2[(size_t)m2 * in.s2 + 1];
            float A[16], x[4], p[3];
            const float P1r0[4] = {K[0], 0.f, K[2], 0.f}, P1r1[4] = {0.f, K[4], K[5], 0.f}, P1r2[4] = {0.f, 0.f, 1.f, 0.f};
            for (int j = 0; j < 4; j++) {   // Triangulate (:738-741)
                A[j] = x1 * P1r2[j] - P1r0[j];
                A[4 + j] = y1 * P1r2[j] - P1r1[j];
                A[8 + j] = x2 * P2[8 + j] - P2[j];
                A[12 + j] = y2 * P2[8 + j] - P2[4 + j];
            }
            svd4_null(A, x);
            const double iw = 1. / (double)x[3];
            for (int k = 0; k < 3; k++) p[k] = (float)((double)x[k] * iw);
            if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) continue;
            const float dist1 = (float)norm3(p);
            const float n2[3] = {p[0] - O2[0], p[1] - O2[1], p[2] - O2[2]};
            const float dist2 = (float)norm3(n2);
            const double dot = ((double)p[0] * (double)n2[0] + (double)p[1] * (double)n2[1]) + (double)p[2] * (double)n2[2];
            const float cosParallax = (float)(dot / (double)(dist1 * dist2));
            if (p[2] <= 0 && (double)cosParallax < 0.99998) continue;
            float q[3];
            for (int k = 0; k < 3; k++)     // R*p3dC1+t
                q[k] = (float)((((double)R[k * 3] * (double)p[0] + (double)R[k * 3 + 1] * (double)p[1]) + (double)R[k * 3 + 2] * (double)p[2]) + (double)t[k]);
            if (q[2] <= 0 && (double)cosParallax < 0.99998) continue;
            const float invZ1 = (float)(1.0 / (double)p[2]);
            const float im1x = in.fx * p[0] * invZ1 + in.cx, im1y = in.fy * p[1] * invZ1 + in.cy;
            const float squareError1 = (im1x - x1) * (im1x - x1) + (im1y - y1) * (im1y - y1);
            if (squareError1 > th2) continue;
            const float invZ2 = (float)(1.0 / (double)q[2]);
            const float im2x = in.fx * q[0] * invZ2 + in.cx, im2y = in.fy * q[1] * invZ2 + in.cy;
            const float squareError2 = (im2x - x2) * (im2x - x2) + (im2y - y2) * (im2y - y2);
            if (squareError2 > th2) continue;
            cc[i] = cosParallax;
            cp[3 * i] = p[0]; cp[3 * i + 1] = p[1]; cp[3 * i + 2] = p[2];
            cf[i] = (uint8_t)(2 | ((double)cosParallax < 0.99998 ? 1 : 0));   // bit 1: counted in nGood, bit 0: vbGood
            mine++;
        }
        if (mine) atomicAdd(&s_cnt[0], mine);
        __syncthreads();
        const int nGood = s_cnt[0];
        float parallax = 0.f;
        if (nGood > 0) {   // sorted vCosParallax[min(50, nGood - 1)] as a rank selection: the smallest key with more than idx keys <= it
            const int idx = nGood - 1 < 50 ? nGood - 1 : 50;
            uint32_t lo = 0u, hi = 0xffffffffu;
            for (int step = 0; step < 32; step++) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                __syncthreads();
                if (tid == 0) s_cnt[1] = 0;
                __syncthreads();
                int below = 0;
                for (int i = tid; i < N; i += INI_BT)
                    if ((cf[i] & 2) && float_key(cc[i]) <= mid) below++;
                if (below) atomicAdd(&s_cnt[1], below);
                __syncthreads();
                if (s_cnt[1] > idx) hi = mid; else lo = mid + 1u;
            }
            parallax = (float)((double)(acosf(key_float(lo)) * 180) / INI_PI);
        }
        __syncthreads();
        if (tid == 0) { s_good[c] = nGood; s_par[c] = parallax; }
        __syncthreads();
    }

    // acceptance
    int win = -1, bestGood = 0, secondBestGood = 0;
    float bestParallax = -1.f;
    bool ok = false;
    if (ncand == 8) {        // :689-731
        for (int i = 0; i < 8; i++) {
            const int nGood = s_good[i];
            if (nGood > bestGood) { secondBestGood = bestGood; bestGood = nGood; win = i; bestParallax = s_par[i]; }
            else if (nGood > secondBestGood) secondBestGood = nGood;
        }
        ok = (double)secondBestGood < 0.75 * bestGood && bestParallax >= in.minParallax && bestGood > in.minTri && (double)bestGood > 0.9 * nInl;
    } else if (ncand == 4) { // :499-568
        int maxGood = s_good[0];
        for (int i = 1; i < 4; i++) maxGood = s_good[i] > maxGood ? s_good[i] : maxGood;
        const int n09 = (int)(0.9 * nInl), nMinGood = n09 > in.minTri ? n09 : in.minTri;
        int nsimilar = 0;
        for (int i = 0; i < 4; i++)
            if ((double)s_good[i] > 0.7 * maxGood) nsimilar++;
        for (int i = 3; i >= 0; i--)
            if (s_good[i] == maxGood) win = i;            // the else-if chain: the first motion that reaches maxGood
        for (int i = 0; i < 4; i++)
            if (i != win && s_good[i] > secondBestGood) secondBestGood = s_good[i];
        bestGood = maxGood; bestParallax = s_par[win];
        ok = !(maxGood < nMinGood || nsimilar > 1) && bestParallax > in.minParallax;
    }
    if (!ok) {
        for (int i = tid; i < N; i += INI_BT) { P3D[3 * i] = 0.f; P3D[3 * i + 1] = 0.f; P3D[3 * i + 2] = 0.f; tri[i] = 0; }
    } else {
        const float *cp = candP + (size_t)win * N * 3;
        const uint8_t *cf = candF + (size_t)win * N;
        for (int i = tid; i < N; i += INI_BT) { P3D[3 * i] = cp[3 * i]; P3D[3 * i + 1] = cp[3 * i + 1]; P3D[3 * i + 2] = cp[3 * i + 2]; tri[i] = cf[i] & 1; }
    }
    if (tid == 0) {
        out->result = ok ? 1 : 0;
        for (int k = 0; k < 9; k++) out->R[k] = ok ? Rc[win][k] : 0.f;
        for (int k = 0; k < 3; k++) out->t[k] = ok ? tc[win][k] : 0.f;
        info->best_good = bestGood; info->second_good = secondBestGood; info->parallax = ncand ? bestParallax : 0.f; info->ncand = ncand;
        for (int c = 0; c < ncand; c++) { info->ngood[c] = s_good[c]; info->cand_parallax[c] = s_par[c]; }
    }
}

#ifndef ORBX_INIT_HOST
// ------------------------------------------------------------------------------------
// host side: this thread's staging pair (orbx_stage.h)
static thread_local StagePair g_is;
void orbx_internal_release_init_scratch() { g_is.release(); }

static int init_check(const char *fn, const void *k1, int n1, const void *k2, int n2, const int32_t *matches, int N, const int32_t *sets,
                      int iterations, float sigma) {
    if (!k1 || !k2 || !matches || !sets || n1 < 1 || n2 < 1) { orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG; }
    if (N < 8) { orbx_set_error("%s: %d matches, 8 are needed", fn, N); return ORBX_ERR_ARG; }
    if (iterations <= 0 || iterations > (1 << 20)) { orbx_set_error("%s: iterations = %d", fn, iterations); return ORBX_ERR_ARG; }
    if (!(sigma > 0.f)) { orbx_set_error("%s: sigma must be positive", fn); return ORBX_ERR_ARG; }
    for (int i = 0; i < N; i++)
        if (matches[2 * i] < 0 || matches[2 * i] >= n1 || matches[2 * i + 1] < 0 || matches[2 * i + 1] >= n2) {
            orbx_set_error("%s: match %d names a keypoint out of range", fn, i); return ORBX_ERR_ARG;
        }
    for (size_t i = 0; i < (size_t)iterations * 8; i++)
        if (sets[i] < 0 || sets[i] >= N) { orbx_set_error("%s: set %d names match %d of %d", fn, (int)(i / 8), sets[i], N); return ORBX_ERR_ARG; }
    return ORBX_OK;
}

// hk1 / hk2 != NULL: packed x y pairs on the host; else dk1 / dk2 are keypoint records in HBM.  full == false: stages 1-3 only.
static int init_run(const float *hk1, const float *hk2, const orbx_keypoint_t *dk1, const orbx_keypoint_t *dk2, int n1, int n2,
                    const int32_t *matches, int N, const int32_t *sets, int iters, const float *K4, float sigma, float minParallax,
                    int minTri, bool full, int *result, float *R21, float *t21, float *P3D, uint8_t *tri, float *scores,
                    uint8_t *inlH, uint8_t *inlF, orbi_init_info_t *info, int device, hipStream_t user, bool useUser) {
    const size_t nh = 2 * (size_t)iters;
    StagePlan pl;
    // upload block: keys1 | keys2 | matches | sets;  download block: info | out | scores | inlBest | P3D | tri;  device only: the rest
    const size_t oK1 = pl.take(hk1 ? (size_t)n1 * 8 : 0), oK2 = pl.take(hk2 ? (size_t)n2 * 8 : 0), oM = pl.take((size_t)N * 8), oS = pl.take((size_t)iters * 32);
    pl.mark_inputs();
    const size_t oInfo = pl.take(sizeof(orbi_init_info_t)), oOut = pl.take(sizeof(InitOut)), oSc = pl.take(nh * 4), oIb = pl.take(2 * (size_t)N);
    const size_t oP = pl.take((size_t)N * 12), oTri = pl.take(N), oDnEnd = pl.off;
    const size_t oNorm = pl.take(sizeof(InitNorm)), oMod = pl.take(nh * 36), oInl = pl.take(nh * N);
    const size_t oCP = pl.take(8 * (size_t)N * 12), oCF = pl.take(8 * (size_t)N), oCC = pl.take(8 * (size_t)N * 4);
    int rc = g_is.reserve(device, pl.off, (size_t)1 << 20);
    if (rc) return rc;
    uint8_t *d = g_is.d, *h = g_is.h;
    const hipStream_t st = useUser ? user : g_is.stream;
    if (hk1) memcpy(h + oK1, hk1, (size_t)n1 * 8);
    if (hk2) memcpy(h + oK2, hk2, (size_t)n2 * 8);
    memcpy(h + oM, matches, (size_t)N * 8);
    memcpy(h + oS, sets, (size_t)iters * 32);
    ORBX_HIP(hipMemcpyAsync(d, h, pl.in_end, hipMemcpyHostToDevice, st));
    InitIn in;
    in.k1 = hk1 ? (const float *)(d + oK1) : (const float *)dk1; in.s1 = hk1 ? 2 : (int)(sizeof(orbx_keypoint_t) / 4);
    in.k2 = hk2 ? (const float *)(d + oK2) : (const float *)dk2; in.s2 = hk2 ? 2 : (int)(sizeof(orbx_keypoint_t) / 4);
    in.n1 = n1; in.n2 = n2; in.matches = (const int32_t *)(d + oM); in.N = N; in.sets = (const int32_t *)(d + oS); in.iters = iters;
    in.sigma = sigma; in.fx = K4 ? K4[0] : 1.f; in.fy = K4 ? K4[1] : 1.f; in.cx = K4 ? K4[2] : 0.f; in.cy = K4 ? K4[3] : 0.f;
    in.minParallax = minParallax; in.minTri = minTri;
    InitNorm *norm = (InitNorm *)(d + oNorm);
    float *models = (float *)(d + oMod), *dsc = (float *)(d + oSc);
    uint8_t *dinl = d + oInl, *dib = d + oIb;
    orbi_init_info_t *dinfo = (orbi_init_info_t *)(d + oInfo);
    (void)hipGetLastError();
    hipLaunchKernelGGL(k_init_normalize, dim3(2), dim3(INI_BT), 0, st, in, norm);
    hipLaunchKernelGGL(k_init_ransac, dim3((unsigned)nh), dim3(INI_RT), 0, st, in, (const InitNorm *)norm, models, dsc, dinl);
    hipLaunchKernelGGL(k_init_select, dim3(1), dim3(INI_BT), 0, st, in, (const float *)models, (const float *)dsc, (const uint8_t *)dinl, dib, dinfo);
    if (full)
        hipLaunchKernelGGL(k_init_reconstruct, dim3(1), dim3(INI_BT), 0, st, in, (const uint8_t *)dib, (float *)(d + oCP), d + oCF,
                           (float *)(d + oCC), dinfo, (InitOut *)(d + oOut), (float *)(d + oP), d + oTri);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(h + oInfo, d + oInfo, (full ? oDnEnd : oP) - oInfo, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    if (info) memcpy(info, h + oInfo, sizeof(orbi_init_info_t));
    if (scores) memcpy(scores, h + oSc, nh * 4);
    if (inlH) memcpy(inlH, h + oIb, N);
    if (inlF) memcpy(inlF, h + oIb + N, N);
    if (full) {
        const InitOut *o = (const InitOut *)(h + oOut);
        *result = o->result;
        memcpy(R21, o->R, 36); memcpy(t21, o->t, 12);
        memcpy(P3D, h + oP, (size_t)N * 12); memcpy(tri, h + oTri, N);
    }
    return ORBX_OK;
}

extern "C" int orbi_initialize(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int N, const int32_t *sets,
                               int iterations, const float *K4, float sigma, float min_parallax, int min_triangulated, int *result,
                               float *R21, float *t21, float *P3D, uint8_t *triangulated, orbi_init_info_t *info, int device) {
    int rc = init_check("orbi_initialize", keys1, n1, keys2, n2, matches, N, sets, iterations, sigma);
    if (rc) return rc;
    if (!K4 || !result || !R21 || !t21 || !P3D || !triangulated) { orbx_set_error("orbi_initialize: bad arguments"); return ORBX_ERR_ARG; }
    return init_run(keys1, keys2, nullptr, nullptr, n1, n2, matches, N, sets, iterations, K4, sigma, min_parallax, min_triangulated, true,
                    result, R21, t21, P3D, triangulated, nullptr, nullptr, nullptr, info, device, nullptr, false);
}

extern "C" int orbi_initialize_device(const orbx_keypoint_t *d_keys1, int n1, const orbx_keypoint_t *d_keys2, int n2,
                                      const int32_t *matches, int N, const int32_t *sets, int iterations, const float *K4, float sigma,
                                      float min_parallax, int min_triangulated, int *result, float *R21, float *t21, float *P3D,
                                      uint8_t *triangulated, orbi_init_info_t *info, int device, void *stream) {
    int rc = init_check("orbi_initialize_device", d_keys1, n1, d_keys2, n2, matches, N, sets, iterations, sigma);
    if (rc) return rc;
    if (!K4 || !result || !R21 || !t21 || !P3D || !triangulated) { orbx_set_error("orbi_initialize_device: bad arguments"); return ORBX_ERR_ARG; }
    return init_run(nullptr, nullptr, d_keys1, d_keys2, n1, n2, matches, N, sets, iterations, K4, sigma, min_parallax, min_triangulated,
                    true, result, R21, t21, P3D, triangulated, nullptr, nullptr, nullptr, info, device, (hipStream_t)stream, true);
}

extern "C" int orbi_search(const float *keys1, int n1, const float *keys2, int n2, const int32_t *matches, int N, const int32_t *sets,
                           int iterations, float sigma, float *scores, uint8_t *inliersH, uint8_t *inliersF, orbi_init_info_t *info,
                           int device) {
    int rc = init_check("orbi_search", keys1, n1, keys2, n2, matches, N, sets, iterations, sigma);
    if (rc) return rc;
    if (!scores || !inliersH || !inliersF) { orbx_set_error("orbi_search: bad arguments"); return ORBX_ERR_ARG; }
    return init_run(keys1, keys2, nullptr, nullptr, n1, n2, matches, N, sets, iterations, nullptr, sigma, 0.f, 0, false, nullptr, nullptr,
                    nullptr, nullptr, nullptr, scores, inliersH, inliersF, info, device, nullptr, false);
}
#endif   // ORBX_INIT_HOST
