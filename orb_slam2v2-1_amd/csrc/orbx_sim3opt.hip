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
// wave_sum, block_sum, quat_from_R, quat_rotate, quat_to_R and the LDL^T are copies of orbx_poseopt.hip's (that file is unchanged).
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

#define S3O_WAVES ((S3O_THREADS + S3O_LANES - 1) / S3O_LANES)
#define S3O_LDS_ROWS 1024   // matches staged in LDS (48 B each, 48 KiB: with the static arrays, 4.2 KiB, under the 64 KiB a launch gets unasked); the rest is read from HBM / L2
#define S3O_NACC 36         // 28 upper entries of H, 7 of b, the robust chi2

struct S3oProblem { int32_t off, n; orbz_sim3_problem_t p; };
struct S3oRow { float P1[3], P2[3], u1, v1, u2, v2, is1, is2; };   // 48 B: the two points in their own camera frames, the keypoints, the informations
struct S3 { double q[4], t[3], s; };                               // q = x y z w

__device__ __forceinline__ double s3o_wave_sum(double v) {
#pragma unroll
    for (int m = S3O_LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, S3O_LANES);   // a + b == b + a bit for bit: every lane ends with the same sum
    return v;
}
template <int K>
__device__ __forceinline__ void s3o_block_sum(double (&a)[K], double *part) {
    const int lane = threadIdx.x % S3O_LANES, wave = threadIdx.x / S3O_LANES;
#pragma unroll
    for (int k = 0; k < K; k++) a[k] = s3o_wave_sum(a[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) part[wave * K + k] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double t = part[k];
#pragma unroll
        for (int w = 1; w < S3O_WAVES; w++) t += part[w * K + k];   // ((w0 + w1) + w2) + w3
        a[k] = t;
    }
}

// Eigen::Quaternion(Matrix3) (Shoemake), as Sim3(R, t, s) and Sim3(Vector7d) use it: no normalisation
__device__ __forceinline__ void s3o_quat_from_R(const double R[9], double q[4]) {
    double t = R[0] + R[4] + R[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > R[i * 4]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
        double v[3];
        v[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
        v[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
        v[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
        q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
    }
}
__device__ __forceinline__ void s3o_quat_rotate(const double q[4], const double v[3], double r[3]) {   // Quaternion * Vector3 (_transformVector)
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    r[0] = (v[0] + q[3] * uv[0]) + (q[1] * uv[2] - q[2] * uv[1]);
    r[1] = (v[1] + q[3] * uv[1]) + (q[2] * uv[0] - q[0] * uv[2]);
    r[2] = (v[2] + q[3] * uv[2]) + (q[0] * uv[1] - q[1] * uv[0]);
}
__device__ __forceinline__ void s3o_quat_to_R(const double q[4], double R[9]) {   // Quaternion::toRotationMatrix
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// Sim3::operator* (sim3.h:266-272): the quaternion product is not normalised
__device__ __forceinline__ S3 s3o_mul(const S3 &a, const S3 &b) {
    S3 r;
    const double ax = a.q[0], ay = a.q[1], az = a.q[2], aw = a.q[3], bx = b.q[0], by = b.q[1], bz = b.q[2], bw = b.q[3];
    r.q[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    r.q[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    r.q[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
    r.q[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
    double rt[3];
    s3o_quat_rotate(a.q, b.t, rt);
    r.t[0] = a.s * rt[0] + a.t[0]; r.t[1] = a.s * rt[1] + a.t[1]; r.t[2] = a.s * rt[2] + a.t[2];
    r.s = a.s * b.s;
    return r;
}
// Sim3::inverse (sim3.h:233-236): (r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
__device__ __forceinline__ S3 s3o_inverse(const S3 &a) {
    S3 r;
    r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
    const double k = -1. / a.s;
    const double v[3] = {k * a.t[0], k * a.t[1], k * a.t[2]};
    s3o_quat_rotate(r.q, v, r.t);
    r.s = 1. / a.s;
    return r;
}
// Sim3(const Vector7d &update) (sim3.h:70-142), update = omega | upsilon | sigma, with its four branches as written.  The numeric
// Jacobian's steps of 1e-9 always take the first (R = I + Omega + Omega^2, A = 1/2, B = 1/6, C = 1): no sin / cos there.
__device__ __forceinline__ S3 s3o_exp(const double u[7]) {
    const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double Om2[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Om2[r * 3 + c] = (Om[r * 3] * Om[c] + Om[r * 3 + 1] * Om[3 + c]) + Om[r * 3 + 2] * Om[6 + c];
    S3 S;
    S.s = exp(sigma);
    const double eps = 0.00001;
    double A, B, Cc, ra, rb;   // R = (I + ra Omega) + rb Omega^2
    if (fabs(sigma) < eps) {
        Cc = 1.0;
        if (theta < eps) {
            A = 1. / 2.; B = 1. / 6.; ra = 1.0; rb = 1.0;
        } else {
            const double theta2 = theta * theta, si = sin(theta), co = cos(theta);
            A = (1.0 - co) / theta2;
            B = (theta - si) / (theta2 * theta);
            ra = si / theta; rb = (1.0 - co) / (theta * theta);
        }
    } else {
        Cc = (S.s - 1.0) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1.0) * S.s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * S.s) / (sigma2 * sigma);
            ra = 1.0; rb = 1.0;
        } else {
            const double si = sin(theta), co = cos(theta);
            ra = si / theta; rb = (1.0 - co) / (theta * theta);
            const double a = S.s * si, b = S.s * co, theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((Cc - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2;
        }
    }
    double R[9], W[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double id = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        R[k] = (id + ra * Om[k]) + rb * Om2[k];
        W[k] = (A * Om[k] + B * Om2[k]) + Cc * id;
    }
    s3o_quat_from_R(R, S.q);
#pragma unroll
    for (int r = 0; r < 3; r++) S.t[r] = (W[r * 3] * u[3] + W[r * 3 + 1] * u[4]) + W[r * 3 + 2] * u[5];
    return S;
}

struct S3oCam { double fx, fy, cx, cy; };
// obs - cam_map(project(S.map(P))) (types_seven_dof_expmap.h:138-167): map is s * (r * xyz) + t, project divides by z unchecked
__device__ __forceinline__ void s3o_error(const S3 &S, const double P[3], double u, double v, const S3oCam &c, double &e0, double &e1) {
    double r[3];
    s3o_quat_rotate(S.q, P, r);
    const double x = S.s * r[0] + S.t[0], y = S.s * r[1] + S.t[1], z = S.s * r[2] + S.t[2];
    e0 = u - ((x / z) * c.fx + c.cx);
    e1 = v - ((y / z) * c.fy + c.cy);
}

// One edge at S: error, chi2, Huber; acc[35] += rho[0].  LIN: + the numeric Jacobian at the 14 perturbed estimates pert[2d] (+delta),
// pert[2d + 1] (-delta) (base_binary_edge.hpp:147-198) and the edge's share of H (28 upper entries, row-major) and b (7) in
// acc[0..34].  Returns the plain chi2 (BaseEdge::chi2).
template <bool LIN>
__device__ __forceinline__ double s3o_edge(const S3 &S, const S3 *pert, const double P[3], double u, double v, const S3oCam &c, double is2,
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
            const S3 Sp = pert[2 * d], Sm = pert[2 * d + 1];
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

// (H + lambda I) x = b by an unpivoted LDL^T in double, orbx_poseopt.hip's solve6 at 7.  false when a pivot is not positive
// (LinearSolverDense: !isPositive()): then x = 0 and the caller leaves the estimate unchanged for that trial.  With a fixed scale
// row / column 6 of H is zero: D[6] = lambda, x[6] = 0 / lambda = 0.  Where Eigen's pivoted LDLT would decide differently (a
// singular H) the behaviour is not pinned.
__device__ __forceinline__ bool s3o_solve7(const double *Hu, const double *b, double lambda, double *x) {
    double A[7][7], L[7][7], D[7];
    int k = 0;
#pragma unroll
    for (int j = 0; j < 7; j++)
#pragma unroll
        for (int l = j; l < 7; l++, k++) { A[j][l] = Hu[k]; A[l][j] = Hu[k]; }
#pragma unroll
    for (int j = 0; j < 7; j++) A[j][j] += lambda;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double d = A[j][j];
#pragma unroll
        for (int m = 0; m < j; m++) d -= (L[j][m] * L[j][m]) * D[m];
        if (!(d > 0.0) || !(d <= DBL_MAX)) ok = false;
        D[j] = d;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double s = A[i][j];
#pragma unroll
            for (int m = 0; m < j; m++) s -= (L[i][m] * L[j][m]) * D[m];
            L[i][j] = s / d;
        }
    }
    double yv[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double s = b[i];
#pragma unroll
        for (int m = 0; m < i; m++) s -= L[i][m] * yv[m];
        yv[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) yv[i] = yv[i] / D[i];
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double s = yv[i];
#pragma unroll
        for (int m = i + 1; m < 7; m++) s -= L[m][i] * x[m];
        x[i] = s;
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 7; i++) x[i] = 0.0;
    }
    return ok;
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
    __shared__ S3 pert[2][14];   // [0]: Sim3(+-delta e_d) * estimate, [1]: their inverses
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
    S3 S0;
    {
        double R[9];
#pragma unroll
        for (int k = 0; k < 9; k++) R[k] = (double)pr.p.R[k];
        s3o_quat_from_R(R, S0.q);
        S0.t[0] = (double)pr.p.t[0]; S0.t[1] = (double)pr.p.t[1]; S0.t[2] = (double)pr.p.t[2];
        S0.s = (double)pr.p.s;
    }
    S3 S = S0;
    int its[2] = {0, 0}, trs[2] = {0, 0}, rounds = 0, nBad = 0, buf = 0;
    bool done = false;   // the second classification ran: the estimate goes out

    // one pass over the thread's live matches at S: edge 12 maps point 2 with S into camera 1, edge 21 point 1 with S^-1 into camera 2
    auto pass = [&](auto lin, const S3 &Sf, double *acc) {
        const S3 Si = s3o_inverse(Sf);
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
                    const S3 Sp = s3o_mul(s3o_exp(upd), S);
                    pert[0][k] = Sp;
                    pert[1][k] = s3o_inverse(Sp);
                }
                __syncthreads();
                double acc[S3O_NACC];
#pragma unroll
                for (int k = 0; k < S3O_NACC; k++) acc[k] = 0.0;
                pass(LinT(), S, acc);
                s3o_block_sum<S3O_NACC>(acc, part[buf]); buf ^= 1;
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
                    const S3 backup = S;
                    double x[7];
                    const bool ok = s3o_solve7(acc, acc + 28, lambda, x);
                    if (fixScale) x[6] = 0.0;   // oplusImpl writes it into the solver's x (types_seven_dof_expmap.h:64-65): computeScale sees the zero
                    if (ok) S = s3o_mul(s3o_exp(x), S);
                    double a1[1], tmpacc[S3O_NACC];
                    tmpacc[35] = 0.0;
                    pass(ErrT(), S, tmpacc);
                    a1[0] = tmpacc[35];
                    s3o_block_sum<1>(a1, part[buf]); buf ^= 1;
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
        const S3 So = done ? S : S0;
        float *to = Sout + (size_t)p * 16;
        double R[9];
        s3o_quat_to_R(So.q, R);   // Converter::toCvMat(g2o::Sim3): toCvMat(s * R, t)
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
