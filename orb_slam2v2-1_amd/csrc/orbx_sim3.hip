// orbx_sim3.hip — Sim3Solver (reference: src/Sim3Solver.cc:37-423) for B problems (loop candidates) as a chain of three launches
// on one stream:
//   k_sim3_prepare   the per-pair part of the constructor (:54-109): X1c, X2c, their images, the two thresholds     pairs / 256 workgroups
//   k_sim3_ransac    one hypothesis per workgroup of one wave: ComputeSim3 (:226-337), CheckInliers (:340-364)      sum of iterations
//   k_sim3_select    the replay of iterate's sequential loop (:158-201) over the stored counts                      B workgroups
// Float where the reference is CV_32F, double where it says double, cv::gemm and cv::norm are csrc/orbx_cvmath.h; cv::eigen is
// csrc/orbx_jacobi_eig.h and cv::Rodrigues is written out below.  DESIGN.md section 6 has the list; tests/sim3_ref.py is the same
// arithmetic in numpy.  No floating-point value crosses lanes: the inlier count is a ballot and a popcount, so the bytes do not
// depend on the launch shape.  Every loop has a bound that is a constant or an argument.
#ifdef ORBX_SIM3_HOST
// tests/cpp/sim3_lockstep.cc compiles the kernels' text for the host as ONE thread per workgroup (tests/cpp/hip_lockstep.h comes
// first) and runs the workgroups one after the other.  Nothing below the kernels is compiled there.
#define S3_RT 1
#define S3_BT 1
#else
#include "orbx_stage.h"
#define S3_RT 64      // k_sim3_ransac: one wave
#define S3_BT 256
#endif
#include <float.h>
#include <math.h>
#include "orbx_cvmath.h"
#include "orbx_jacobi_eig.h"

struct Sim3Rec { float X1c[3], X2c[3], p1[2], p2[2], thr1, thr2; };   // 48 B per pair
// all arrays on the device; problem b owns pairs off[b] .. off[b+1]-1 and hypotheses soff[b] .. soff[b+1]-1, its flags start at
// fbase[b] (= sum over the problems before it of iterations x pairs)
struct Sim3In {
    const orbs_pair_t *pairs; const orbs_problem_t *prob; const int32_t *off, *soff, *sets, *pprob, *hprob; const int64_t *fbase;
    int B, npairs, nhyp;
};

// Rcw*X+tcw as one cv::gemm with its addend: the sum of gemv3 (orbx_cvmath.h), + t in double, narrowed once.  T: the top three rows of a
// row-major 4x4 (stride 4)
__device__ __forceinline__ void s3_transform(const float *T, const float *X, float *d) {
    for (int k = 0; k < 3; k++)
        d[k] = (float)((((double)T[k * 4] * (double)X[0] + (double)T[k * 4 + 1] * (double)X[1]) + (double)T[k * 4 + 2] * (double)X[2]) + (double)T[k * 4 + 3]);
}
// mvnMaxError (:87-88) is a std::vector<size_t>: 9.210*sigmaSquare in double, truncated; the comparison converts it to float.
// At or above 2^64 (no pyramid has such a level) the conversion is pinned to 2^64.
__device__ __forceinline__ float s3_threshold(float sigma2) {
    const double v = 9.210 * (double)sigma2;
    return v >= 18446744073709551616.0 ? 18446744073709551616.0f : (float)(unsigned long long)v;
}

__global__ __launch_bounds__(S3_BT) void k_sim3_prepare(Sim3In in, Sim3Rec *__restrict__ recs) {
    for (int i = blockIdx.x * S3_BT + threadIdx.x; i < in.npairs; i += gridDim.x * S3_BT) {
        const orbs_pair_t pr = in.pairs[i];
        const orbs_problem_t *pb = in.prob + in.pprob[i];
        Sim3Rec r;
        s3_transform(pb->Tcw1, pr.w1, r.X1c);
        s3_transform(pb->Tcw2, pr.w2, r.X2c);
        pinhole_image(r.X1c, pb->K1, r.p1);
        pinhole_image(r.X2c, pb->K2, r.p2);
        r.thr1 = s3_threshold(pr.sigma2_1);
        r.thr2 = s3_threshold(pr.sigma2_2);
        recs[i] = r;
    }
}

// ComputeCentroid (:215-224): cv::reduce(SUM) over the 3 columns of a row keeps two float accumulators, (x0 + x2) + x1; C/P.cols is
// C * (1./3) in double, narrowed
__device__ __forceinline__ void s3_centroid(const float *P, float *Pr, float *O) {
    for (int r = 0; r < 3; r++) {
        const float sum = (P[r * 3] + P[r * 3 + 2]) + P[r * 3 + 1];
        O[r] = (float)((double)sum * (1. / 3));
        for (int c = 0; c < 3; c++) Pr[r * 3 + c] = P[r * 3 + c] - O[r];
    }
}

// ---- one hypothesis per workgroup.  Every lane forms the model itself from the three pairs of the set: all branches are uniform.
__global__ __launch_bounds__(S3_RT) void k_sim3_ransac(Sim3In in, const Sim3Rec *__restrict__ recs, float *__restrict__ models,
                                                       int32_t *__restrict__ counts, uint8_t *__restrict__ flags) {
    const int tid = threadIdx.x, hyp = blockIdx.x, b = in.hprob[hyp];
    const int first = in.off[b], n = in.off[b + 1] - first, it = hyp - in.soff[b];
    const orbs_problem_t pb = in.prob[b];
    const Sim3Rec *rec = recs + first;
    float P1[9], P2[9], Pr1[9], Pr2[9], O1[3], O2[3];
    for (int c = 0; c < 3; c++) {   // mvX3Dc[idx].copyTo(P3Dci.col(c))
        const Sim3Rec *s = rec + in.sets[(size_t)hyp * 3 + c];
        for (int r = 0; r < 3; r++) { P1[r * 3 + c] = s->X1c[r]; P2[r * 3 + c] = s->X2c[r]; }
    }
    s3_centroid(P1, Pr1, O1);
    s3_centroid(P2, Pr2, O2);
    float M[9];
    gemm33<true>(Pr2, Pr1, M);      // M = Pr2*Pr1.t()
    // the N entries are float expressions (M.at<float>() + M.at<float>() is float arithmetic) held in doubles and narrowed back (:251-265)
    const float N11 = M[0] + M[4] + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3];
    const float N22 = M[0] - M[4] - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2];
    const float N33 = -M[0] + M[4] - M[8], N34 = M[5] + M[7], N44 = -M[0] - M[4] + M[8];
    const float Nm[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float eval[4], evec[16];
    jacobi_eig4(Nm, eval, evec);    // evec row 0: the quaternion of the rotation
    float vec[3] = {evec[1], evec[2], evec[3]};
    const double nv = norm3(vec);
    const double ang = atan2(nv, (double)evec[0]);
    const double alpha = (2 * ang) * (1. / nv);       // vec = 2*ang*vec/norm(vec): 0/0 for a zero imaginary part, unguarded
    for (int k = 0; k < 3; k++) vec[k] = (float)((double)vec[k] * alpha);
    float R[9];
    {   // cv::Rodrigues on the float 3-vector, in double
        const double rx = (double)vec[0], ry = (double)vec[1], rz = (double)vec[2];
        const double theta = sqrt((rx * rx + ry * ry) + rz * rz);
        if (theta < DBL_EPSILON) {
            for (int k = 0; k < 9; k++) R[k] = (k % 4 == 0) ? 1.f : 0.f;
        } else {
            const double c = cos(theta), s = sin(theta), c1 = 1. - c;
            const double kx = rx / theta, ky = ry / theta, kz = rz / theta;
            const double kk[9] = {kx * kx, kx * ky, kx * kz, ky * kx, ky * ky, ky * kz, kz * kx, kz * ky, kz * kz};
            const double Kx[9] = {0., -kz, ky, kz, 0., -kx, -ky, kx, 0.};
            for (int k = 0; k < 9; k++) R[k] = (float)((c * ((k % 4 == 0) ? 1. : 0.) + c1 * kk[k]) + s * Kx[k]);
        }
    }
    float ms = 1.0f;
    if (!pb.fix_scale) {            // :292-309
        float P3[9];
        gemm33(R, Pr2, P3);         // P3 = mR12i*Pr2
        double nom = 0.0, den = 0.0;
        for (int k = 0; k < 9; k++) nom += (double)Pr1[k] * (double)P3[k];
        for (int k = 0; k < 9; k++) den += (double)(P3[k] * P3[k]);   // cv::pow(P3, 2) squares in float
        ms = (float)(nom / den);
    }
    float t[3], T12[16], T21[16];
    for (int k = 0; k < 3; k++) {   // O1 - ms12i*mR12i*O2: one gemm, alpha = -s, + O1 in double
        const double acc = ((double)R[k * 3] * (double)O2[0] + (double)R[k * 3 + 1] * (double)O2[1]) + (double)R[k * 3 + 2] * (double)O2[2];
        t[k] = (float)((double)O1[k] - acc * (double)ms);
    }
    const double inv_s = 1.0 / (double)ms;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            T12[i * 4 + j] = (float)((double)R[i * 3 + j] * (double)ms);      // sR = ms12i*mR12i
            T21[i * 4 + j] = (float)((double)R[j * 3 + i] * inv_s);           // sRinv = (1.0/ms12i)*mR12i.t()
        }
        T12[i * 4 + 3] = t[i];
    }
    gemv3(T21, t, T21 + 3, -1.0, 4, 4);   // tinv = -sRinv*mt12i
    for (int j = 0; j < 4; j++) { T12[12 + j] = T21[12 + j] = (j == 3) ? 1.f : 0.f; }
    if (tid == 0) {
        float *m = models + (size_t)hyp * 13;
        m[0] = ms;
        for (int k = 0; k < 9; k++) m[1 + k] = R[k];
        for (int k = 0; k < 3; k++) m[10 + k] = t[k];
    }

    // CheckInliers (:340-364): pair i belongs to lane i % 64
    uint8_t *fl = flags + in.fbase[b] + (int64_t)it * n;
    int cnt = 0;
    for (int base = 0; base < n; base += S3_RT) {
        const int i = base + tid;
        bool inl = false;
        if (i < n) {
            const Sim3Rec r = rec[i];
            float q[3], P2im1[2], P1im2[2];
            s3_transform(T12, r.X2c, q); pinhole_image(q, pb.K1, P2im1);
            s3_transform(T21, r.X1c, q); pinhole_image(q, pb.K2, P1im2);
            const float d1x = r.p1[0] - P2im1[0], d1y = r.p1[1] - P2im1[1];
            const float d2x = P1im2[0] - r.p2[0], d2y = P1im2[1] - r.p2[1];
            const float err1 = (float)((double)d1x * (double)d1x + (double)d1y * (double)d1y);
            const float err2 = (float)((double)d2x * (double)d2x + (double)d2y * (double)d2y);
            inl = err1 < r.thr1 && err2 < r.thr2;    // a NaN compares false
            fl[i] = inl ? 1 : 0;
        }
        cnt += __popcll(__ballot(inl));
    }
    if (tid == 0) counts[hyp] = cnt;
}

// ---- iterate's loop (:158-201) over the counts of one problem per workgroup
__global__ __launch_bounds__(S3_BT) void k_sim3_select(Sim3In in, const float *__restrict__ models, const int32_t *__restrict__ counts,
                                                      const uint8_t *__restrict__ flags, uint8_t *__restrict__ hitInl,
                                                      orbs_sim3_info_t *__restrict__ infos) {
    __shared__ int s_hit;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int first = in.off[b], n = in.off[b + 1] - first, h0 = in.soff[b], its = in.soff[b + 1] - h0;
    if (tid == 0) {
        const int minInl = in.prob[b].min_inliers;
        int hit = -1, best = -1, bestInl = 0;
        for (int it = 0; it < its; it++) {
            const int c = counts[h0 + it];
            if (c >= bestInl) {
                bestInl = c; best = it;
                if (c > minInl) { hit = it; break; }
            }
        }
        s_hit = hit;
        orbs_sim3_info_t o;
        o.n = n; o.iterations = its; o.hit_iteration = hit; o.best_iteration = best; o.best_inliers = bestInl;
        o.s = 0.f;
        for (int k = 0; k < 9; k++) o.R[k] = 0.f;
        for (int k = 0; k < 3; k++) o.t[k] = 0.f;
        for (int k = 0; k < 16; k++) o.T12[k] = 0.f;
        if (best >= 0) {
            const float *m = models + (size_t)(h0 + best) * 13;
            o.s = m[0];
            for (int k = 0; k < 9; k++) o.R[k] = m[1 + k];
            for (int k = 0; k < 3; k++) o.t[k] = m[10 + k];
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) o.T12[i * 4 + j] = (float)((double)m[1 + i * 3 + j] * (double)m[0]);
                o.T12[i * 4 + 3] = m[10 + i];
            }
            o.T12[15] = 1.f;
        }
        infos[b] = o;
    }
    __syncthreads();
    const int hit = s_hit;
    const uint8_t *src = flags + in.fbase[b] + (int64_t)(hit < 0 ? 0 : hit) * n;
    for (int i = tid; i < n; i += S3_BT) hitInl[first + i] = hit < 0 ? 0 : src[i];
}

#ifndef ORBX_SIM3_HOST
// ------------------------------------------------------------------------------------
// host side: this thread's staging pair (orbx_stage.h)
static thread_local StagePair g_ss;
void orbx_internal_release_sim3_scratch() { g_ss.release(); }
#define S3_MAX_TOTAL (1 << 24)      // pairs, and hypotheses, of one call

extern "C" int orbs_sim3_iterations(int n, double probability, int min_inliers, int max_iterations) {
    if (n < min_inliers) return 0;
    const float epsilon = (float)min_inliers / n;
    int nIterations;
    if (min_inliers == n)
        nIterations = 1;
    else {   // nIterations = ceil(...) converts a double to int: kept in range here, where the reference's conversion is undefined
        const double k = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        nIterations = !(k < (double)max_iterations) ? max_iterations : (k < 1.0 ? 1 : (int)k);
    }
    return std::max(1, std::min(nIterations, max_iterations));
}

extern "C" int orbs_sim3_ransac_batch(const orbs_pair_t *pairs, const int32_t *offsets, int B, const orbs_problem_t *problems,
                                      const int32_t *sets, const int32_t *set_offsets, int32_t *counts, float *models, uint8_t *flags,
                                      uint8_t *hit_inliers, orbs_sim3_info_t *infos, int device) {
    const char *fn = "orbs_sim3_ransac_batch";
    if (!pairs || !offsets || !problems || !sets || !set_offsets || !counts || !hit_inliers || !infos || B < 0) {
        orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG;
    }
    if (B == 0) return ORBX_OK;
    if (offsets[0] < 0 || set_offsets[0] < 0) { orbx_set_error("%s: negative offset", fn); return ORBX_ERR_ARG; }
    size_t nflags = 0;
    for (int b = 0; b < B; b++) {
        const int n = offsets[b + 1] - offsets[b], its = set_offsets[b + 1] - set_offsets[b];
        if (offsets[b + 1] < offsets[b] || set_offsets[b + 1] < set_offsets[b]) { orbx_set_error("%s: offsets decrease at problem %d", fn, b); return ORBX_ERR_ARG; }
        if (offsets[b + 1] > S3_MAX_TOTAL || set_offsets[b + 1] > S3_MAX_TOTAL) { orbx_set_error("%s: more than %d pairs or sets", fn, S3_MAX_TOTAL); return ORBX_ERR_ARG; }
        if (its > 0 && n < 3) { orbx_set_error("%s: problem %d has %d pairs, 3 are needed", fn, b, n); return ORBX_ERR_ARG; }
        for (int i = offsets[b]; i < offsets[b + 1]; i++) {
            const float s1 = pairs[i].sigma2_1, s2 = pairs[i].sigma2_2;
            if (!(s1 >= 0.f) || !(s2 >= 0.f) || !std::isfinite(s1) || !std::isfinite(s2)) {
                orbx_set_error("%s: pair %d of problem %d has a sigma2 that is negative or not finite", fn, i - offsets[b], b); return ORBX_ERR_ARG;
            }
        }
        for (int h = set_offsets[b]; h < set_offsets[b + 1]; h++) {
            const int32_t *s = sets + (size_t)h * 3;
            if (s[0] < 0 || s[0] >= n || s[1] < 0 || s[1] >= n || s[2] < 0 || s[2] >= n) {
                orbx_set_error("%s: set %d of problem %d names a pair out of %d", fn, h - set_offsets[b], b, n); return ORBX_ERR_ARG;
            }
            if (s[0] == s[1] || s[0] == s[2] || s[1] == s[2]) {
                orbx_set_error("%s: set %d of problem %d names a pair twice", fn, h - set_offsets[b], b); return ORBX_ERR_ARG;
            }
        }
        nflags += (size_t)its * n;
    }
    if (nflags > ((size_t)1 << 31)) { orbx_set_error("%s: %zu flag bytes", fn, nflags); return ORBX_ERR_ARG; }
    const int p0 = offsets[0], h0 = set_offsets[0], np = offsets[B] - p0, nh = set_offsets[B] - h0;   // the arrays' used ranges start at offsets[0]
    StagePlan pl;
    // upload block: pairs | problems | off | soff | sets | pprob | hprob | fbase;  download block: infos | counts | hit | models | flags;
    // device only: the records
    const size_t oPa = pl.take((size_t)np * sizeof(orbs_pair_t)), oPr = pl.take((size_t)B * sizeof(orbs_problem_t));
    const size_t oOf = pl.take(((size_t)B + 1) * 4), oSo = pl.take(((size_t)B + 1) * 4), oSe = pl.take((size_t)nh * 12);
    const size_t oPp = pl.take((size_t)np * 4), oHp = pl.take((size_t)nh * 4), oFb = pl.take((size_t)B * 8);
    pl.mark_inputs();
    const size_t oInfo = pl.take((size_t)B * sizeof(orbs_sim3_info_t)), oCnt = pl.take((size_t)nh * 4), oHit = pl.take((size_t)np);
    const size_t oMod = pl.take((size_t)nh * 52), oFl = pl.take(nflags), oDnEnd = pl.off;
    const size_t oRec = pl.take((size_t)np * sizeof(Sim3Rec));
    int rc = g_ss.reserve(device, pl.off, (size_t)1 << 20);
    if (rc) return rc;
    uint8_t *d = g_ss.d, *h = g_ss.h;
    const hipStream_t st = g_ss.stream;
    memcpy(h + oPa, pairs + p0, (size_t)np * sizeof(orbs_pair_t));
    memcpy(h + oPr, problems, (size_t)B * sizeof(orbs_problem_t));
    memcpy(h + oSe, sets + (size_t)h0 * 3, (size_t)nh * 12);
    int32_t *hOf = (int32_t *)(h + oOf), *hSo = (int32_t *)(h + oSo), *hPp = (int32_t *)(h + oPp), *hHp = (int32_t *)(h + oHp);
    int64_t *hFb = (int64_t *)(h + oFb);
    int64_t fb = 0;
    for (int b = 0; b < B; b++) {
        hOf[b] = offsets[b] - p0; hSo[b] = set_offsets[b] - h0; hFb[b] = fb;
        for (int i = offsets[b]; i < offsets[b + 1]; i++) hPp[i - p0] = b;
        for (int k = set_offsets[b]; k < set_offsets[b + 1]; k++) hHp[k - h0] = b;
        fb += (int64_t)(set_offsets[b + 1] - set_offsets[b]) * (offsets[b + 1] - offsets[b]);
    }
    hOf[B] = np; hSo[B] = nh;
    ORBX_HIP(hipMemcpyAsync(d, h, pl.in_end, hipMemcpyHostToDevice, st));
    Sim3In in;
    in.pairs = (const orbs_pair_t *)(d + oPa); in.prob = (const orbs_problem_t *)(d + oPr); in.off = (const int32_t *)(d + oOf);
    in.soff = (const int32_t *)(d + oSo); in.sets = (const int32_t *)(d + oSe); in.pprob = (const int32_t *)(d + oPp);
    in.hprob = (const int32_t *)(d + oHp); in.fbase = (const int64_t *)(d + oFb); in.B = B; in.npairs = np; in.nhyp = nh;
    Sim3Rec *recs = (Sim3Rec *)(d + oRec);
    float *dmod = (float *)(d + oMod);
    int32_t *dcnt = (int32_t *)(d + oCnt);
    (void)hipGetLastError();
    if (np > 0 && nh > 0) {
        const int g = (np + S3_BT - 1) / S3_BT;
        hipLaunchKernelGGL(k_sim3_prepare, dim3((unsigned)(g < 1024 ? g : 1024)), dim3(S3_BT), 0, st, in, recs);
        hipLaunchKernelGGL(k_sim3_ransac, dim3((unsigned)nh), dim3(S3_RT), 0, st, in, (const Sim3Rec *)recs, dmod, dcnt, d + oFl);
    }
    hipLaunchKernelGGL(k_sim3_select, dim3((unsigned)B), dim3(S3_BT), 0, st, in, (const float *)dmod, (const int32_t *)dcnt,
                       (const uint8_t *)(d + oFl), d + oHit, (orbs_sim3_info_t *)(d + oInfo));
    ORBX_HIP(hipGetLastError());
    const size_t dnEnd = flags ? oDnEnd : (models ? oFl : oMod);
    ORBX_HIP(hipMemcpyAsync(h + oInfo, d + oInfo, dnEnd - oInfo, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    memcpy(infos, h + oInfo, (size_t)B * sizeof(orbs_sim3_info_t));
    memcpy(counts + h0, h + oCnt, (size_t)nh * 4);
    memcpy(hit_inliers + p0, h + oHit, (size_t)np);
    if (models) memcpy(models + (size_t)h0 * 13, h + oMod, (size_t)nh * 52);
    if (flags) memcpy(flags, h + oFl, nflags);
    return ORBX_OK;
}

extern "C" int orbs_sim3_ransac(const orbs_pair_t *pairs, int n, const orbs_problem_t *problem, const int32_t *sets, int iterations,
                                int32_t *counts, float *models, uint8_t *flags, uint8_t *hit_inliers, orbs_sim3_info_t *info, int device) {
    if (n < 0 || iterations < 0) { orbx_set_error("orbs_sim3_ransac: n = %d, iterations = %d", n, iterations); return ORBX_ERR_ARG; }
    const int32_t off[2] = {0, n}, soff[2] = {0, iterations};
    return orbs_sim3_ransac_batch(pairs, off, 1, problem, sets, soff, counts, models, flags, hit_inliers, info, device);
}
#endif   // ORBX_SIM3_HOST
