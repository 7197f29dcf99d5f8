// orbx_poseopt.hip — Optimizer::PoseOptimization (reference: src/Optimizer.cc:239-451) as one kernel launch: one 6-DoF vertex, N unary
// reprojection edges, 4 rounds x <= 10 Levenberg-Marquardt iterations x <= 10 trials, a 6x6 solve per trial.  A restatement of the
// reference and of the g2o classes it drives (types_six_dof_expmap, se3quat.h, optimization_algorithm_levenberg, base_unary_edge,
// robust_kernel_impl (Huber), sparse_optimizer::optimize, linear_solver_dense), double throughout with the reference's float
// narrowings; DESIGN.md section 6 has the list.  tests/pose_ref.py is the same arithmetic in numpy, statement for statement.
//
// One workgroup per problem.  Edge i belongs to thread i % 256 for the whole call, so an edge's state (its flag, the chi2 of its last
// evaluation) is only ever touched by one thread.  Every pass over the edges ends in block_sum: the thread's own edges in ascending
// order, then a butterfly over the wave, then the four waves in order - a fixed order, no floating-point atomics, so two runs give
// the same bits.  After a sum every thread holds the same doubles and runs the solve and the LM control flow redundantly: all
// branches are uniform without a broadcast, and every loop has a compile-time bound (4 rounds, 10 iterations, 10 trials).
#ifdef ORBX_POSEOPT_HOST
// tests/cpp/poseopt_lockstep.cc compiles the kernel's text for the host as ONE thread (tests/cpp/hip_lockstep.h comes first): the
// thread's edges in ascending order are then the whole sum, which is tests/pose_ref.py's order - the two must agree
// bit for bit (tests/test_poseopt_cpu.py).  Nothing below the kernel is compiled there.
#define PO_THREADS 1
#define PO_LANES 1
#else
#include "orbx_stage.h"
#define PO_THREADS 256
#define PO_LANES 64
#endif
#include <float.h>
#include <math.h>
#include "orbx_g2omath.h"

#define PO_WAVES ((PO_THREADS + PO_LANES - 1) / PO_LANES)
#define PO_LDS_EDGES 1536   // observations staged in LDS (32 B each, 48 KiB: with the static arrays under the 64 KiB a launch gets unasked); the rest is read from HBM / L2
#define PO_NACC 28          // 21 upper entries of H, 6 of b, the robust chi2

struct PoseProblem { int32_t off, n; orbm_camera_t cam; float Tcw[16]; };
// the device form's sources: Frame arrays left in HBM by extraction, and the map-point positions
struct PoseDevSrc { const orbx_keypoint_t *kun; const float *uright; const orbo_worldpos_t *pts; float is2[ORBX_MAX_LEVELS]; int nlevels; float dMono, dStereo; };
struct Se3 { double t[3], q[4]; };   // q = x y z w
struct PoCam { double fx, fy, cx, cy, bf; float dMono, dStereo; };
// block_sum, the quaternion functions, se3_oplus and the LDL^T are orbx_g2omath.h's

// One edge at pose T: project, error, chi2, Huber; LIN: + its share of H (21 upper entries, row-major), b (6) in acc[0..26].
// acc[27] += rho[0].  Returns the plain chi2 (BaseEdge::chi2).  A monocular edge is the stereo one with a zero third row.
template <bool LIN>
__device__ __forceinline__ double edge_eval(const orbo_observation_t &o, const PoCam &c, const Se3 &T, bool robust, double *acc) {
    const double Xw[3] = {(double)o.wx, (double)o.wy, (double)o.wz};
    double X[3];
    quat_rotate(T.q, Xw, X);
    const double x = X[0] + T.t[0], y = X[1] + T.t[1], z = X[2] + T.t[2];
    const bool mono = o.ur < 0.f;
    double e0, e1, e2;
    if (mono) {   // project2d, then * f + c, in double
        e0 = (double)o.u - ((x / z) * c.fx + c.cx);
        e1 = (double)o.v - ((y / z) * c.fy + c.cy);
        e2 = 0.0;
    } else {      // const float invz = 1.0f / trans_xyz[2]   (types_six_dof_expmap.cpp:299-306)
        const double iz = (double)(float)(1.0 / z);
        const double pu = (x * iz) * c.fx + c.cx;
        e0 = (double)o.u - pu;
        e1 = (double)o.v - ((y * iz) * c.fy + c.cy);
        e2 = (double)o.ur - (pu - c.bf * iz);
    }
    const double is2 = (double)o.inv_sigma2;
    const double oe0 = is2 * e0, oe1 = is2 * e1, oe2 = is2 * e2;
    const double chi2 = (e0 * oe0 + e1 * oe1) + e2 * oe2;
    const double delta = mono ? (double)c.dMono : (double)c.dStereo;   // (float)sqrt(5.991), (float)sqrt(7.815), widened (:273-274)
    const double dsqr = delta * delta;
    double rho0 = chi2, w = 1.0;
    if (robust && !(chi2 <= dsqr)) {
        const double s = sqrt(chi2);
        rho0 = (2.0 * s) * delta - dsqr;
        w = delta / s;
    }
    acc[27] += rho0;
    if (LIN) {
        const double invz = 1.0 / z, invz2 = invz * invz;
        double J[3][6];
        J[0][0] = ((x * y) * invz2) * c.fx;
        J[0][1] = -(1.0 + ((x * x) * invz2)) * c.fx;
        J[0][2] = (y * invz) * c.fx;
        J[0][3] = -invz * c.fx;
        J[0][4] = 0.0;
        J[0][5] = (x * invz2) * c.fx;
        J[1][0] = (1.0 + (y * y) * invz2) * c.fy;
        J[1][1] = ((-x * y) * invz2) * c.fy;
        J[1][2] = (-x * invz) * c.fy;
        J[1][3] = 0.0;
        J[1][4] = -invz * c.fy;
        J[1][5] = (y * invz2) * c.fy;
        if (mono) {
#pragma unroll
            for (int j = 0; j < 6; j++) J[2][j] = 0.0;
        } else {
            J[2][0] = J[0][0] - (c.bf * y) * invz2;
            J[2][1] = J[0][1] + (c.bf * x) * invz2;
            J[2][2] = J[0][2];
            J[2][3] = J[0][3];
            J[2][4] = 0.0;
            J[2][5] = J[0][5] - c.bf * invz2;
        }
        const double wo = w * is2;   // robustInformation: rho[1] * information, the second-order term is commented out
        int k = 0;
#pragma unroll
        for (int j = 0; j < 6; j++) {
#pragma unroll
            for (int l = j; l < 6; l++, k++)
                acc[k] += ((J[0][j] * wo) * J[0][l] + (J[1][j] * wo) * J[1][l]) + (J[2][j] * wo) * J[2][l];
        }
#pragma unroll
        for (int j = 0; j < 6; j++) acc[21 + j] -= w * ((J[0][j] * oe0 + J[1][j] * oe1) + J[2][j] * oe2);
    }
    return chi2;
}

__global__ __launch_bounds__(PO_THREADS) void k_pose_opt(const PoseProblem *__restrict__ probs, const orbo_observation_t *__restrict__ obs,
                                                         PoseDevSrc src, uint8_t *__restrict__ outl, float *__restrict__ chi,
                                                         float *__restrict__ Tout, int32_t *__restrict__ ngood,
                                                         orbo_pose_info_t *__restrict__ infos) {
    extern __shared__ __align__(16) uint8_t po_lds[];
    __shared__ double part[2][PO_WAVES * PO_NACC];
    __shared__ int cnt[2];
    orbo_observation_t *cache = (orbo_observation_t *)po_lds;
    const int tid = threadIdx.x, p = blockIdx.x;
    const PoseProblem pr = probs[p];
    const int off = pr.off, n = pr.n, ncache = n < PO_LDS_EDGES ? n : PO_LDS_EDGES;
    const PoCam cam = {(double)pr.cam.fx, (double)pr.cam.fy, (double)pr.cam.cx, (double)pr.cam.cy, (double)pr.cam.mbf, src.dMono, src.dStereo};
    uint8_t *fl = outl + off;
    float *ch = chi + off;

    auto fetch = [&](int i) -> orbo_observation_t {   // edge i from the call's source
        if (src.kun) {
            const orbo_worldpos_t w = src.pts[i];
            const orbx_keypoint_t kp = src.kun[i];
            int oc = kp.octave;
            oc = oc < 0 ? 0 : (oc >= src.nlevels ? src.nlevels - 1 : oc);
            orbo_observation_t o = {w.valid, kp.x, kp.y, src.uright[i], src.is2[oc], w.wx, w.wy, w.wz};
            return o;
        }
        return obs[off + i];
    };
    auto load = [&](int i) -> orbo_observation_t { return i < ncache ? cache[i] : fetch(i); };
    if (tid < 2) cnt[tid] = 0;
    __syncthreads();
    {   // stage the observations, count the correspondences, clear their flags (:289, :323)
        int mine = 0;
        for (int i = tid; i < n; i += PO_THREADS) {
            const orbo_observation_t o = fetch(i);
            if (i < ncache) cache[i] = o;
            if (o.valid) { mine++; fl[i] = 0; }
        }
        if (mine) atomicAdd(&cnt[0], mine);
    }
    __syncthreads();
    const int nInit = cnt[0];

    // Converter::toSE3Quat(mTcw): SE3Quat(R, t) from the float 4x4
    Se3 T0;
    {
        double R[9];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) R[r * 3 + c] = (double)pr.Tcw[r * 4 + c];
            T0.t[r] = (double)pr.Tcw[r * 4 + 3];
        }
        quat_from_R(R, T0.q);
        normalize_rotation(T0.q);
    }
    Se3 T = T0;
    int its[4] = {0, 0, 0, 0}, trs[4] = {0, 0, 0, 0}, rounds = 0, nBad = 0, buf = 0;

    if (nInit >= 3) {
        for (int round = 0; round < 4; round++) {
            T = T0;   // every round restarts from the input pose (:377)
            const bool robust = round <= 2;   // setRobustKernel(0) after round index 2 (:407, :436)
            double lambda = 0.0, ni = 2.0;
            int nbadIt = 0;
            for (int it = 0; it < 10; it++) {
                double acc[PO_NACC];
#pragma unroll
                for (int k = 0; k < PO_NACC; k++) acc[k] = 0.0;
                for (int i = tid; i < n; i += PO_THREADS) {
                    const orbo_observation_t o = load(i);
                    if (o.valid && !fl[i]) ch[i] = (float)edge_eval<true>(o, cam, T, robust, acc);
                }
                block_sum<PO_LANES, PO_WAVES>(acc, part[buf]); buf ^= 1;
                double cur = acc[27];
                const double iniChi = cur;
                if (it == 0) {   // computeLambdaInit: tau * max |diag H|
                    double md = 0.0;
                    md = fmax(fabs(acc[0]), md); md = fmax(fabs(acc[6]), md); md = fmax(fabs(acc[11]), md);
                    md = fmax(fabs(acc[15]), md); md = fmax(fabs(acc[18]), md); md = fmax(fabs(acc[20]), md);
                    lambda = 1e-5 * md; ni = 2.0; nbadIt = 0;
                }
                double rho = 0.0;
                int q = 0;
                for (int trial = 0; trial < 10; trial++) {
                    const Se3 backup = T;
                    double x[6];
                    const bool ok = ldlt_solve<6>(acc, acc + 21, lambda, x);
                    if (ok) se3_oplus(T.t, T.q, x);
                    double a1[1] = {0.0}, tmpacc[PO_NACC];
                    tmpacc[27] = 0.0;
                    for (int i = tid; i < n; i += PO_THREADS) {
                        const orbo_observation_t o = load(i);
                        if (o.valid && !fl[i]) ch[i] = (float)edge_eval<false>(o, cam, T, robust, tmpacc);
                    }
                    a1[0] = tmpacc[27];
                    block_sum<PO_LANES, PO_WAVES>(a1, part[buf]); buf ^= 1;
                    double tmp = a1[0];
                    if (!ok) tmp = DBL_MAX;
                    double scale = 0.0;
#pragma unroll
                    for (int j = 0; j < 6; j++) scale += x[j] * (lambda * x[j] + acc[21 + j]);
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
                        T = backup;
                    }
                    q++;
                    if (!(rho < 0.0)) break;
                }
                its[round]++; trs[round] += q;
                if (q == 10 || rho == 0.0) break;
                if ((iniChi - cur) * 1e3 < iniChi) nbadIt++; else nbadIt = 0;   // the reference's own stop criterion
                if (nbadIt >= 3) break;
            }
            // classify (:382-438): an active edge keeps the chi2 of its last evaluation, a flagged one is evaluated at the round's pose
            int bad = 0;
            for (int i = tid; i < n; i += PO_THREADS) {
                const orbo_observation_t o = load(i);
                if (!o.valid) continue;
                float c2;
                if (fl[i]) { double dummy[PO_NACC]; dummy[27] = 0.0; c2 = (float)edge_eval<false>(o, cam, T, false, dummy); }
                else c2 = ch[i];
                const bool flag = c2 > (o.ur < 0.f ? 5.991f : 7.815f);
                fl[i] = flag ? 1 : 0;
                bad += flag ? 1 : 0;
            }
            if (tid == 0) cnt[1] = 0;
            __syncthreads();
            if (bad) atomicAdd(&cnt[1], bad);
            __syncthreads();
            nBad = cnt[1];
            __syncthreads();
            rounds = round + 1;
            if (nInit < 10) break;   // optimizer.edges().size() < 10: the total, not the active count (:440)
        }
    }
    if (tid == 0) {
        float *to = Tout + (size_t)p * 16;
        if (nInit >= 3) {
            double R[9];
            quat_to_R(T.q, R);
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) to[r * 4 + c] = (float)R[r * 3 + c];
                to[r * 4 + 3] = (float)T.t[r];
            }
            to[12] = 0.f; to[13] = 0.f; to[14] = 0.f; to[15] = 1.f;
            ngood[p] = nInit - nBad;
        } else {
            for (int k = 0; k < 16; k++) to[k] = pr.Tcw[k];
            ngood[p] = 0;
        }
        orbo_pose_info_t inf;
        inf.correspondences = nInit; inf.bad = nBad; inf.rounds = rounds;
        for (int r = 0; r < 4; r++) { inf.iterations[r] = its[r]; inf.trials[r] = trs[r]; }
        for (int r = 0; r < 3; r++) inf.t[r] = T.t[r];
        for (int r = 0; r < 4; r++) inf.q[r] = T.q[r];
        infos[p] = inf;
    }
}

#ifndef ORBX_POSEOPT_HOST
// ------------------------------------------------------------------------------------
// host side: this thread's staging pair (orbx_stage.h)
static thread_local StagePair g_ps;
void orbx_internal_release_pose_scratch() { g_ps.release(); }

// obs == NULL: the device form (src holds the HBM arrays, pts the host records of the one problem)
static int pose_run(const orbo_observation_t *obs, const int32_t *offsets, int B, const orbm_camera_t *cams, const float *Tin,
                    float *Tout, uint8_t *outlier, int32_t *ngood, orbo_pose_info_t *infos, int device, PoseDevSrc src,
                    const orbo_worldpos_t *pts, hipStream_t user, bool useUser) {
    const size_t total = (size_t)offsets[B], nmax = total > 0 ? total : 1;
    StagePlan pl;
    // upload block: problems | observations (or world positions) | flags;  download block: flags | poses | ngood | infos;  device only: chi2
    const size_t oProb = pl.take((size_t)B * sizeof(PoseProblem)), oObs = pl.take(nmax * (obs ? sizeof(orbo_observation_t) : sizeof(orbo_worldpos_t)));
    const size_t oFl = pl.take(nmax), oT = pl.take((size_t)B * 64), oNg = pl.take((size_t)B * 4), oInf = pl.take((size_t)B * sizeof(orbo_pose_info_t));
    const size_t oChi = pl.take(nmax * 4);
    src.dMono = (float)sqrt(5.991); src.dStereo = (float)sqrt(7.815);
    int rc = g_ps.reserve(device, pl.off, (size_t)1 << 18);
    if (rc) return rc;
    uint8_t *d = g_ps.d, *h = g_ps.h;
    const hipStream_t st = useUser ? user : g_ps.stream;
    PoseProblem *hp = (PoseProblem *)(h + oProb);
    int nbig = 0;
    for (int b = 0; b < B; b++) {
        hp[b].off = offsets[b]; hp[b].n = offsets[b + 1] - offsets[b]; hp[b].cam = cams[b];
        memcpy(hp[b].Tcw, Tin + (size_t)b * 16, 64);
        if (hp[b].n > nbig) nbig = hp[b].n;
    }
    if (obs) memcpy(h + oObs, obs, total * sizeof(orbo_observation_t));
    else memcpy(h + oObs, pts, total * sizeof(orbo_worldpos_t));
    memcpy(h + oFl, outlier, total);
    ORBX_HIP(hipMemcpyAsync(d, h, oFl + nmax, hipMemcpyHostToDevice, st));
    if (!obs) src.pts = (const orbo_worldpos_t *)(d + oObs);
    (void)hipGetLastError();
    const size_t lds = (size_t)(nbig < PO_LDS_EDGES ? nbig : PO_LDS_EDGES) * sizeof(orbo_observation_t);
    hipLaunchKernelGGL(k_pose_opt, dim3(B), dim3(PO_THREADS), lds, st, (const PoseProblem *)(d + oProb),
                       (const orbo_observation_t *)(obs ? d + oObs : nullptr), src, d + oFl, (float *)(d + oChi), (float *)(d + oT),
                       (int32_t *)(d + oNg), (orbo_pose_info_t *)(d + oInf));
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipMemcpyAsync(h + oFl, d + oFl, oChi - oFl, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    memcpy(outlier, h + oFl, total);
    memcpy(Tout, h + oT, (size_t)B * 64);
    memcpy(ngood, h + oNg, (size_t)B * 4);
    if (infos) memcpy(infos, h + oInf, (size_t)B * sizeof(orbo_pose_info_t));
    return ORBX_OK;
}

extern "C" int orbo_pose_optimization_batch(const orbo_observation_t *obs, const int32_t *offsets, int B, const orbm_camera_t *cams,
                                            const float *Tcw_in16, float *Tcw_out16, uint8_t *outlier, int32_t *ngood,
                                            orbo_pose_info_t *infos, int device) {
    if (B < 0 || !offsets || (B > 0 && (!cams || !Tcw_in16 || !Tcw_out16 || !ngood))) {
        orbx_set_error("orbo_pose_optimization_batch: bad arguments"); return ORBX_ERR_ARG;
    }
    if (offsets[0] < 0) { orbx_set_error("orbo_pose_optimization_batch: negative offset"); return ORBX_ERR_ARG; }
    for (int b = 0; b < B; b++)
        if (offsets[b + 1] < offsets[b]) { orbx_set_error("orbo_pose_optimization_batch: offsets are not monotone"); return ORBX_ERR_ARG; }
    if (offsets[B] > 0 && (!obs || !outlier)) { orbx_set_error("orbo_pose_optimization_batch: bad arguments"); return ORBX_ERR_ARG; }
    if (B == 0) return ORBX_OK;
    PoseDevSrc src;
    memset(&src, 0, sizeof(src));
    static const orbo_observation_t none = {0, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint8_t nofl = 0;
    return pose_run(obs ? obs : &none, offsets, B, cams, Tcw_in16, Tcw_out16, outlier ? outlier : &nofl, ngood, infos, device, src, nullptr,
                    nullptr, false);
}

extern "C" int orbo_pose_optimization(const orbo_observation_t *obs, int n, const orbm_camera_t *cam, const float *Tcw_in16,
                                      float *Tcw_out16, uint8_t *outlier, int *ngood, orbo_pose_info_t *info, int device) {
    if (n < 0 || !cam || !Tcw_in16 || !Tcw_out16 || !ngood || (n > 0 && (!obs || !outlier))) {
        orbx_set_error("orbo_pose_optimization: bad arguments"); return ORBX_ERR_ARG;
    }
    const int32_t offsets[2] = {0, n};
    int32_t ng = 0;
    const int rc = orbo_pose_optimization_batch(obs, offsets, 1, cam, Tcw_in16, Tcw_out16, outlier, &ng, info, device);
    if (rc == ORBX_OK) *ngood = ng;
    return rc;
}

extern "C" int orbo_pose_optimization_device(const orbx_keypoint_t *d_kun, const float *d_uright, int n, const float *inv_level_sigma2,
                                             int nlevels, const orbo_worldpos_t *pts, const orbm_camera_t *cam, const float *Tcw_in16,
                                             float *Tcw_out16, uint8_t *outlier, int *ngood, orbo_pose_info_t *info, int device,
                                             void *stream) {
    if (n < 0 || !cam || !Tcw_in16 || !Tcw_out16 || !ngood || !inv_level_sigma2 || nlevels < 1 || nlevels > ORBX_MAX_LEVELS ||
        (n > 0 && (!d_kun || !d_uright || !pts || !outlier))) {
        orbx_set_error("orbo_pose_optimization_device: bad arguments"); return ORBX_ERR_ARG;
    }
    const int32_t offsets[2] = {0, n};
    if (n == 0) {   // nothing in HBM to read: the host-array form on an empty problem
        int32_t ng = 0;
        const int rc = orbo_pose_optimization_batch(nullptr, offsets, 1, cam, Tcw_in16, Tcw_out16, nullptr, &ng, info, device);
        if (rc == ORBX_OK) *ngood = ng;
        return rc;
    }
    PoseDevSrc src;
    memset(&src, 0, sizeof(src));
    src.kun = d_kun; src.uright = d_uright; src.nlevels = nlevels;
    for (int l = 0; l < nlevels; l++) src.is2[l] = inv_level_sigma2[l];
    int32_t ng = 0;
    const int rc = pose_run(nullptr, offsets, 1, cam, Tcw_in16, Tcw_out16, outlier, &ng, info, device, src, pts, (hipStream_t)stream, true);
    if (rc == ORBX_OK) *ngood = ng;
    return rc;
}
#endif   // ORBX_POSEOPT_HOST
