// orbx_sim3opt.hip — Optimizer::OptimizeSim3 (reference: src/Optimizer.cc:1051-1246) as one kernel launch: one free 7-DoF vertex
// (VertexSim3Expmap), two reprojection edges per match (EdgeSim3ProjectXYZ, EdgeInverseSim3ProjectXYZ) whose map-point vertices are
// all fixed, a dense 7x7 solve: 2 rounds x <= 10 Levenberg-Marquardt iterations x <= 10 trials.  A restatement of the reference and
// of the g2o classes it drives (types_seven_dof_expmap, sim3.h, base_binary_edge.hpp's NUMERIC linearizeOplus - the analytic one is
// commented out in the reference -, optimization_algorithm_levenberg, robust_kernel_impl (Huber), linear_solver_dense), double
// throughout with the reference's float narrowings; DESIGN.md section 6 has the list.  tests/sim3opt_ref.py is the same arithmetic
// in numpy, statement for statement.
//
// The shape is k_pose_opt's (orbx_poseopt.hip): one workgroup per problem, match m belongs to thread m % 256 for the whole call, so
// a match's state (its flag, whether its last evaluation exceeded th2) is only ever touched by one thread.  Every pass over the
// matches ends in block_sum: the thread's own matches in ascending order, then a butterfly over the wave, then the four waves in
// order - a fixed order, no floating-point atomics, so two runs give the same bits.  After a sum every thread holds the same doubles
// and runs the solve and the LM control flow redundantly; every loop has a compile-time bound (2 rounds, 10 iterations, 10 trials,
// 14 perturbations).  The numeric Jacobian is taken at the vertex, as g2o's push / oplus / pop does: per linearisation the 14
// estimates Sim3(+-delta e_d) * estimate and their inverses are the same for every edge; 14 threads form them once into LDS.
// block_sum, the quaternion and Sim3 functions and the LDL^T are orbx_g2omath.h's.
#ifdef ORBX_SIM3OPT_HOST
// tests/cpp/sim3opt_lockstep.cc compiles the kernel's text for the host as ONE thread (tests/cpp/hip_lockstep.h comes first): the
// thread's matches in ascending order are then the whole sum, which is tests/sim3opt_ref.py's order - the two must agree bit for
// bit (tests/test_sim3opt_cpu.py).  Of the host side only the argument checks are compiled there.
#define S3O_THREADS 1
#define S3O_LANES 1
#else
#include "orbx_stage.h"
#define S3O_THREADS 256
#define S3O_LANES 64
#endif
#include <float.h>
#include <math.h>
#include <type_traits>
#include "orbx_g2omath.h"

#define S3O_WAVES ((S3O_THREADS + S3O_LANES - 1) / S3O_LANES)
#define S3O_LDS_ROWS 1024   // matches staged in LDS (48 B each, 48 KiB: with the static arrays, 4.2 KiB, under the 64 KiB a launch gets unasked); the rest is read from HBM / L2
#define S3O_NACC 36         // 28 upper entries of H, 7 of b, the robust chi2

struct S3oProblem { int32_t off, n; orbz_sim3_problem_t p; };
struct S3oRow { float P1[3], P2[3], u1, v1, u2, v2, is1, is2; };   // 48 B: the two points in their own camera frames, the keypoints, the informations
struct S3oCam { double fx, fy, cx, cy; };
// obs - cam_map(project(S.map(P))) (types_seven_dof_expmap.h:138-167): map is s * (r * xyz) + t, project divides by z unchecked
__device__ __forceinline__ void s3o_error(const orbg_sim3_t &S, const double P[3], double u, double v, const S3oCam &c, double &e0, double &e1) {
    double X[3];
    sim3_map(S, P, X);
    const double x = X[0], y = X[1], z = X[2];
    e0 = u - ((x / z) * c.fx + c.cx);
    e1 = v - ((y / z) * c.fy + c.cy);
}

// One edge at S: error, chi2, Huber; acc[35] += rho[0].  LIN: + the numeric Jacobian at the 14 perturbed estimates pert[2d] (+delta),
// pert[2d + 1] (-delta) (base_binary_edge.hpp:147-198) and the edge's share of H (28 upper entries, row-major) and b (7) in
// acc[0..34].  Returns the plain chi2 (BaseEdge::chi2).
template <bool LIN>
__device__ __forceinline__ double s3o_edge(const orbg_sim3_t &S, const orbg_sim3_t *pert, const double P[3], double u, double v, const S3oCam &c, double is2,
                                           double delta, double *acc) {
    double e0, e1;
    s3o_error(S, P, u, v, c, e0, e1);
    const double oe0 = is2 * e0, oe1 = is2 * e1;
    const double chi2 = e0 * oe0 + e1 * oe1;
    const double dsqr = delta * delta;
    double rho0 = chi2, w = 1.0;
    if (!(chi2 <= dsqr)) {
        const double s = sqrt(chi2);
        rho0 = (2.0 * s) * delta - dsqr;
        w = delta / s;
    }
    acc[35] += rho0;
    if (LIN) {
        const double scalar = 1.0 / (2 * 1e-9);
        double J0[7], J1[7];
#pragma unroll
        for (int d = 0; d < 7; d++) {
            double p0, p1, m0, m1;
            const orbg_sim3_t Sp = pert[2 * d], Sm = pert[2 * d + 1];
            s3o_error(Sp, P, u, v, c, p0, p1);
            s3o_error(Sm, P, u, v, c, m0, m1);
            J0[d] = scalar * (p0 - m0);
            J1[d] = scalar * (p1 - m1);
        }
        const double wo = w * is2;   // robustInformation: rho[1] * information
        int k = 0;
#pragma unroll
        for (int j = 0; j < 7; j++) {
#pragma unroll
            for (int l = j; l < 7; l++, k++) acc[k] += (J0[j] * wo) * J0[l] + (J1[j] * wo) * J1[l];
        }
#pragma unroll
        for (int j = 0; j < 7; j++) acc[28 + j] -= w * (J0[j] * oe0 + J1[j] * oe1);
    }
    return chi2;
}

// R*P+t of a cv::Mat expression on CV_32F: one cv::gemm with its addend - the products widened to double, summed left to right,
// + t in double, narrowed once (orbx_sim3.hip's s3_transform; csrc/orbx_cvmath.h has the rules).  T: a row-major 4x4
__device__ __forceinline__ void s3o_transform(const float *T, const float *X, float *d) {
    for (int k = 0; k < 3; k++)
        d[k] = (float)((((double)T[k * 4] * (double)X[0] + (double)T[k * 4 + 1] * (double)X[1]) + (double)T[k * 4 + 2] * (double)X[2]) + (double)T[k * 4 + 3]);
}

__global__ __launch_bounds__(S3O_THREADS) void k_sim3_opt(const S3oProblem *__restrict__ probs, const orbz_sim3_match_t *__restrict__ matches,
                                                          S3oRow *__restrict__ rows, uint8_t *__restrict__ over,
                                                          uint8_t *__restrict__ dropped, float *__restrict__ Sout,
                                                          int32_t *__restrict__ ninl, orbz_sim3_info_t *__restrict__ infos) {
    extern __shared__ __align__(16) uint8_t s3o_lds[];
    __shared__ double part[2][S3O_WAVES * S3O_NACC];
    __shared__ orbg_sim3_t pert[2][14];   // [0]: Sim3(+-delta e_d) * estimate, [1]: their inverses
    __shared__ int cnt[1];
    S3oRow *cache = (S3oRow *)s3o_lds;
    const int tid = threadIdx.x, p = blockIdx.x;
    const S3oProblem pr = probs[p];
    const int off = pr.off, n = pr.n, ncache = n < S3O_LDS_ROWS ? n : S3O_LDS_ROWS;
    const S3oCam cam1 = {(double)pr.p.K1[0], (double)pr.p.K1[1], (double)pr.p.K1[2], (double)pr.p.K1[3]};
    const S3oCam cam2 = {(double)pr.p.K2[0], (double)pr.p.K2[1], (double)pr.p.K2[2], (double)pr.p.K2[3]};
    const double th2 = (double)pr.p.th2;
    const double delta = (double)(float)sqrt((double)pr.p.th2);   // const float deltaHuber = sqrt(th2) (:1100)
    const bool fixScale = pr.p.fix_scale != 0;
    uint8_t *dr = dropped + off, *ov = over + off;
    S3oRow *rw = rows + off;

    auto load = [&](int i) -> S3oRow { return i < ncache ? cache[i] : rw[i]; };
    // stage the matches: the two points into their camera frames in float (:1122-1132), flags cleared
    for (int i = tid; i < n; i += S3O_THREADS) {
        const orbz_sim3_match_t m = matches[off + i];
        S3oRow r;
        s3o_transform(pr.p.Tcw1, m.w1, r.P1);
        s3o_transform(pr.p.Tcw2, m.w2, r.P2);
        r.u1 = m.u1; r.v1 = m.v1; r.u2 = m.u2; r.v2 = m.v2; r.is1 = m.inv_sigma2_1; r.is2 = m.inv_sigma2_2;
        if (i < ncache) cache[i] = r; else rw[i] = r;
        dr[i] = 0; ov[i] = 0;
    }
    __syncthreads();

    // g2o::Sim3 gScm(Converter::toMatrix3d(R), Converter::toVector3d(t), s): Quaterniond(R) of the widened floats, not normalised
    orbg_sim3_t S0;
    {
        double R[9];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = (double)pr.p.R[k];
        quat_from_R(R, S0.q);
        S0.t[0] = (double)pr.p.t[0]; S0.t[1] = (double)pr.p.t[1]; S0.t[2] = (double)pr.p.t[2];
        S0.s = (double)pr.p.s;
    }
    orbg_sim3_t S = S0;
    int its[2] = {0, 0}, trs[2] = {0, 0}, rounds = 0, nBad = 0, buf = 0;
    bool done = false;   // the second classification ran: the estimate goes out

    // one pass over the thread's live matches at S: edge 12 maps point 2 with S into camera 1, edge 21 point 1 with S^-1 into camera 2
    auto pass = [&](auto lin, const orbg_sim3_t &Sf, double *acc) {
        const orbg_sim3_t Si = sim3_inverse(Sf);
        for (int i = tid; i < n; i += S3O_THREADS) {
            if (dr[i]) continue;
            const S3oRow r = load(i);
            bool exceeds = false;
#pragma unroll 1
            for (int e = 0; e < 2; e++) {   // one after the other through ONE copy of the edge's code: both unrolled side by side spilled 258 VGPRs
                const float *Pf = e ? r.P1 : r.P2;
                const double P[3] = {(double)Pf[0], (double)Pf[1], (double)Pf[2]};
                const double c2 = s3o_edge<decltype(lin)::value>(e ? Si : Sf, pert[e], P, (double)(e ? r.u2 : r.u1), (double)(e ? r.v2 : r.v1),
                                                                 e ? cam2 : cam1, (double)(e ? r.is2 : r.is1), delta, acc);
                exceeds = exceeds || c2 > th2;
            }
            ov[i] = exceeds ? 1 : 0;   // e12->chi2()>th2 || e21->chi2()>th2 on the last evaluation (:1198, :1232)
        }
    };
    typedef std::true_type LinT;     // a linearisation: errors, numeric Jacobians, H and b
    typedef std::false_type ErrT;    // a trial: errors only

    if (n >= 1) {
        for (int round = 0; round < 2; round++) {
            const int maxit = round == 0 ? 5 : (nBad > 0 ? 10 : 5);   // optimize(5), then optimize(nMoreIterations) from where the first ended
            double lambda = 0.0, ni = 2.0;
            int nbadIt = 0;
            for (int it = 0; it < 10; it++) {
                if (it >= maxit) break;
                // the vertex side of the numeric Jacobian: oplus(+-delta e_d) is Sim3(update) * estimate, update[6] = 0 with a fixed scale
                for (int k = tid; k < 14; k += S3O_THREADS) {
                    double upd[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    const int d = k >> 1;
#pragma unroll
                    for (int j = 0; j < 7; j++)
                        if (j == d) upd[j] = (k & 1) ? -1e-9 : 1e-9;
                    if (fixScale) upd[6] = 0.0;
                    const orbg_sim3_t Sp = sim3_mul(sim3_exp(upd), S);
                    pert[0][k] = Sp;
                    pert[1][k] = sim3_inverse(Sp);
                }
                __syncthreads();
                double acc[S3O_NACC];
#pragma unroll
                for (int k = 0; k < S3O_NACC; k++) acc[k] = 0.0;
                pass(LinT(), S, acc);
                block_sum<S3O_LANES, S3O_WAVES>(acc, part[buf]); buf ^= 1;
                double cur = acc[35];
                const double iniChi = cur;
                if (it == 0) {   // computeLambdaInit: tau * max |diag H|, at iteration 0 of each optimize()
                    double md = 0.0;
                    md = fmax(fabs(acc[0]), md); md = fmax(fabs(acc[7]), md); md = fmax(fabs(acc[13]), md); md = fmax(fabs(acc[18]), md);
                    md = fmax(fabs(acc[22]), md); md = fmax(fabs(acc[25]), md); md = fmax(fabs(acc[27]), md);
                    lambda = 1e-5 * md; ni = 2.0; nbadIt = 0;
                }
                double rho = 0.0;
                int q = 0;
                for (int trial = 0; trial < 10; trial++) {
                    const orbg_sim3_t backup = S;
                    double x[7];
                    const bool ok = ldlt_solve<7>(acc, acc + 28, lambda, x);
                    if (fixScale) x[6] = 0.0;   // oplusImpl writes it into the solver's x (types_seven_dof_expmap.h:64-65): computeScale sees the zero
                    if (ok) S = sim3_mul(sim3_exp(x), S);
                    double a1[1], tmpacc[S3O_NACC];
                    tmpacc[35] = 0.0;
                    pass(ErrT(), S, tmpacc);
                    a1[0] = tmpacc[35];
                    block_sum<S3O_LANES, S3O_WAVES>(a1, part[buf]); buf ^= 1;
                    double tmp = a1[0];
                    if (!ok) tmp = DBL_MAX;
                    double scale = 0.0;
#pragma unroll
                    for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + acc[28 + j]);
                    scale += 1e-3;
                    rho = (cur - tmp) / scale;
                    if (rho > 0.0 && fabs(tmp) <= DBL_MAX) {
                        const double u = 2.0 * rho - 1.0;
                        double alpha = 1.0 - (u * u) * u;
                        alpha = fmin(alpha, 2.0 / 3.0);
                        lambda *= fmax(1.0 / 3.0, alpha);
                        ni = 2.0;
                        cur = tmp;
                    } else {
                        lambda *= ni;
                        ni *= 2.0;
                        S = backup;
                    }
                    q++;
                    if (!(rho < 0.0)) break;
                }
                its[round]++; trs[round] += q;
                if (q == 10 || rho == 0.0) break;
                if ((iniChi - cur) * 1e3 < iniChi) nbadIt++; else nbadIt = 0;   // the reference's own stop criterion
                if (nbadIt >= 3) break;
            }
            // classify (:1190-1208, :1224-1239): a live match whose last evaluation exceeded th2 on either edge is dropped
            int bad = 0;
            for (int i = tid; i < n; i += S3O_THREADS) {
                if (dr[i]) continue;
                if (ov[i]) { dr[i] = 1; bad++; }
            }
            if (tid == 0) cnt[0] = 0;
            __syncthreads();
            if (bad) atomicAdd(&cnt[0], bad);
            __syncthreads();
            nBad += cnt[0];
            __syncthreads();
            rounds = round + 1;
            if (round == 1) done = true;
            if (n - nBad < 10) break;   // nCorrespondences-nBad<10: return 0, the drops applied, the Sim3 as it came in (:1216-1217)
        }
    }
    if (tid == 0) {
        const orbg_sim3_t So = done ? S : S0;
        float *to = Sout + (size_t)p * 16;
        double R[9];
        quat_to_R(So.q, R);   // Converter::toCvMat(g2o::Sim3): toCvMat(s * R, t)
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) to[r * 4 + c] = (float)(So.s * R[r * 3 + c]);
            to[r * 4 + 3] = (float)So.t[r];
        }
        to[12] = 0.f; to[13] = 0.f; to[14] = 0.f; to[15] = 1.f;
        ninl[p] = done ? n - nBad : 0;
        orbz_sim3_info_t inf;
        inf.correspondences = n; inf.bad = nBad; inf.rounds = rounds; inf.reserved = 0;
        for (int r = 0; r < 2; r++) { inf.iterations[r] = its[r]; inf.trials[r] = trs[r]; }
        for (int r = 0; r < 4; r++) inf.q[r] = So.q[r];
        for (int r = 0; r < 3; r++) inf.t[r] = So.t[r];
        inf.s = So.s;
        infos[p] = inf;
    }
}

// ------------------------------------------------------------------------------------
// the argument checks, before a device is touched (compiled for the host-only test program too)
static int s3o_check(const char *fn, const orbz_sim3_match_t *m, const int32_t *offsets, int B, const orbz_sim3_problem_t *ps, float *S12_out16,
                     uint8_t *dropped, int32_t *ninliers) {
    if (B < 0 || !offsets || (B > 0 && (!ps || !S12_out16 || !ninliers))) { orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG; }
    if (offsets[0] < 0) { orbx_set_error("%s: negative offset", fn); return ORBX_ERR_ARG; }
    for (int b = 0; b < B; b++)
        if (offsets[b + 1] < offsets[b]) { orbx_set_error("%s: offsets are not monotone", fn); return ORBX_ERR_ARG; }
    if (B > 0 && offsets[B] > offsets[0] && (!m || !dropped)) { orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG; }
    for (int b = 0; b < B; b++)
        if (!(ps[b].th2 >= 0.f) || !(ps[b].th2 <= FLT_MAX)) { orbx_set_error("%s: th2 is negative or not finite", fn); return ORBX_ERR_ARG; }
    if (B > 0)
        for (int i = offsets[0]; i < offsets[B]; i++)
            if (!(m[i].inv_sigma2_1 >= 0.f) || !(m[i].inv_sigma2_1 <= FLT_MAX) || !(m[i].inv_sigma2_2 >= 0.f) || !(m[i].inv_sigma2_2 <= FLT_MAX)) {
                orbx_set_error("%s: inv_sigma2 is negative or not finite", fn); return ORBX_ERR_ARG;
            }
    return ORBX_OK;
}

#ifndef ORBX_SIM3OPT_HOST
// host side: this thread's staging pair (orbx_stage.h)
static thread_local StagePair g_so;
void orbx_internal_release_sim3opt_scratch() { g_so.release(); }

extern "C" int orbz_optimize_sim3_batch(const orbz_sim3_match_t *m, const int32_t *offsets, int B, const orbz_sim3_problem_t *ps,
                                        float *S12_out16, uint8_t *dropped, int32_t *ninliers, orbz_sim3_info_t *infos, int device) {
    const int crc = s3o_check("orbz_optimize_sim3_batch", m, offsets, B, ps, S12_out16, dropped, ninliers);
    if (crc) return crc;
    if (B == 0) return ORBX_OK;
    const size_t first = (size_t)offsets[0], total = (size_t)offsets[B] - first, nmax = total > 0 ? total : 1;
    StagePlan pl;
    // upload block: problems | matches;  download block: dropped | Sim3 matrices | ninliers | infos;  device only: rows past the LDS stage | last-evaluation flags
    const size_t oProb = pl.take((size_t)B * sizeof(S3oProblem)), oM = pl.take(nmax * sizeof(orbz_sim3_match_t));
    const size_t oDr = pl.take(nmax), oS = pl.take((size_t)B * 64), oNi = pl.take((size_t)B * 4), oInf = pl.take((size_t)B * sizeof(orbz_sim3_info_t));
    const size_t oRows = pl.take(nmax * sizeof(S3oRow)), oOv = pl.take(nmax);
    (void)oOv;
    int rc = g_so.reserve(device, pl.off, (size_t)1 << 18);
    if (rc) return rc;
    uint8_t *d = g_so.d, *h = g_so.h;
    const hipStream_t st = g_so.stream;
    S3oProblem *hp = (S3oProblem *)(h + oProb);
    int nbig = 0;
    for (int b = 0; b < B; b++) {
        hp[b].off = (int32_t)((size_t)offsets[b] - first); hp[b].n = offsets[b + 1] - offsets[b]; hp[b].p = ps[b];
        if (hp[b].n > nbig) nbig = hp[b].n;
    }
    if (total) memcpy(h + oM, m + first, total * sizeof(orbz_sim3_match_t));
    ORBX_HIP(hipMemcpyAsync(d, h, oDr, hipMemcpyHostToDevice, st));
    (void)hipGetLastError();
    const size_t lds = (size_t)(nbig < S3O_LDS_ROWS ? nbig : S3O_LDS_ROWS) * sizeof(S3oRow);
    hipLaunchKernelGGL(k_sim3_opt, dim3(B), dim3(S3O_THREADS), lds, st, (const S3oProblem *)(d + oProb), (const orbz_sim3_match_t *)(d + oM),
                       (S3oRow *)(d + oRows), d + oOv, d + oDr, (float *)(d + oS), (int32_t *)(d + oNi), (orbz_sim3_info_t *)(d + oInf));
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(h + oDr, d + oDr, oRows - oDr, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    if (total) memcpy(dropped + first, h + oDr, total);
    memcpy(S12_out16, h + oS, (size_t)B * 64);
    memcpy(ninliers, h + oNi, (size_t)B * 4);
    if (infos) memcpy(infos, h + oInf, (size_t)B * sizeof(orbz_sim3_info_t));
    return ORBX_OK;
}

extern "C" int orbz_optimize_sim3(const orbz_sim3_match_t *m, int n, const orbz_sim3_problem_t *p, float *S12_out16, uint8_t *dropped,
                                  int *ninliers, orbz_sim3_info_t *info, int device) {
    if (n < 0 || !p || !S12_out16 || !ninliers || (n > 0 && (!m || !dropped))) {
        orbx_set_error("orbz_optimize_sim3: bad arguments"); return ORBX_ERR_ARG;
    }
    const int32_t offsets[2] = {0, n};
    int32_t ni = 0;
    const int rc = orbz_optimize_sim3_batch(m, offsets, 1, p, S12_out16, dropped, &ni, info, device);
    if (rc == ORBX_OK) *ninliers = ni;
    return rc;
}
#endif   // ORBX_SIM3OPT_HOST
