// orbx_g2omath.h — the g2o / Eigen arithmetic the four device optimisers share, in double as g2o evaluates it: Eigen's quaternion
// expressions, SE3Quat's and Sim3's exponentials and products, the dense LDL^T of LinearSolverDense, and the deterministic double
// sums every pass over the edges ends in.  Every function here is a bit-parity obligation against the g2o / Eigen code its comment
// names: the expression trees, their parentheses and the order of operations are the contract.  The numpy
// restatements (tests/pose_ref.py, tests/sim3opt_ref.py, tests/lba_ref.py, tests/essential_ref.py) state the same trees, and
// tests/cpp/g2omath_check.cc compares the two function by function (tests/test_g2omath_cpu.py).  What has one user (an edge's
// error and Jacobian, Sim3::log, the Huber step with its per-file condition) stays with that user.
// Users: orbx_poseopt.hip, orbx_sim3opt.hip, orbx_lba.hip, orbx_essential.hip.
// No HIP header: tests/cpp/*_lockstep.cc compile this as plain C++ after tests/cpp/hip_lockstep.h; a HIP build includes it after
// the runtime's header (orbx_stage.h brings it).  Quaternions are x y z w; matrices are row-major.
#pragma once
#include <float.h>
#include <math.h>
#include "orbx.h"

// ------------------------------------------------------------------------------------
// Deterministic sums over a workgroup of WAVES waves of LANES lanes: the thread's own terms first (the caller's loop), then a
// butterfly over the wave, then the waves in order - a fixed order, no floating-point atomics, so two runs give the same bits and
// every thread ends with the same doubles.  With LANES = 1 (the lockstep programs) the butterfly has no steps.
// part: WAVES * K doubles of LDS.  block_sum has ONE barrier, between writing part and reading it; the caller owns the barrier
// before part is written again (two sums in a row alternate between two parts, or have a barrier of the caller's in between).
template <int LANES>
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int m = LANES / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, LANES);   // a + b == b + a bit for bit: every lane ends with the same sum
    return v;
}
template <int LANES, int WAVES, int K>
__device__ __forceinline__ void block_sum(double (&a)[K], double *part) {
    const int lane = threadIdx.x % LANES, wave = threadIdx.x / LANES;
#pragma unroll
    for (int k = 0; k < K; k++) a[k] = wave_sum<LANES>(a[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; k++) part[wave * K + k] = a[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; k++) {
        double t = part[k];
#pragma unroll
        for (int w = 1; w < WAVES; w++) t += part[w * K + k];   // ((w0 + w1) + w2) + w3
        a[k] = t;
    }
}
template <int LANES, int WAVES>
__device__ __forceinline__ double block_sum(double v, double *part) {   // one sum: block_sum at K = 1
    double a[1] = {v};
    block_sum<LANES, WAVES, 1>(a, part);
    return a[0];
}

// ------------------------------------------------------------------------------------
// Eigen::Quaternion(Matrix3) (Shoemake), as SE3Quat(R, t), SE3Quat::exp, Sim3(R, t, s) and Sim3(Vector7d) use it: no
// normalisation.  The branch of a non-positive trace is written once per largest diagonal entry I, so that no array is indexed by
// a variable (a variable index puts R and q into scratch memory).
template <int I>
__device__ __forceinline__ void quat_from_R_case(const double R[9], double q[4]) {
    constexpr int J = (I + 1) % 3, K = (J + 1) % 3;
    double t = sqrt(R[I * 4] - R[J * 4] - R[K * 4] + 1.0);
    q[I] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[K * 3 + J] - R[J * 3 + K]) * t;
    q[J] = (R[J * 3 + I] + R[I * 3 + J]) * t;
    q[K] = (R[K * 3 + I] + R[I * 3 + K]) * t;
}
__device__ __forceinline__ void quat_from_R(const double R[9], double q[4]) {
    double t = R[0] + R[4] + R[8];
    if (t > 0.0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i ? R[4] : R[0])) i = 2;
        if (i == 0) quat_from_R_case<0>(R, q);
        else if (i == 1) quat_from_R_case<1>(R, q);
        else quat_from_R_case<2>(R, q);
    }
}
__device__ __forceinline__ void normalize_rotation(double q[4]) {   // se3quat.h:280-285
    if (q[3] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] /= n; q[1] /= n; q[2] /= n; q[3] /= n;
}
__device__ __forceinline__ void quat_rotate(const double q[4], const double v[3], double r[3]) {   // Quaternion * Vector3 (_transformVector)
    double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
    uv[0] += uv[0]; uv[1] += uv[1]; uv[2] += uv[2];
    r[0] = (v[0] + q[3] * uv[0]) + (q[1] * uv[2] - q[2] * uv[1]);
    r[1] = (v[1] + q[3] * uv[1]) + (q[2] * uv[0] - q[0] * uv[2]);
    r[2] = (v[2] + q[3] * uv[2]) + (q[0] * uv[1] - q[1] * uv[0]);
}
__device__ __forceinline__ void quat_to_R(const double q[4], double R[9]) {   // Quaternion::toRotationMatrix
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}
// Quaternion * Quaternion (the Hamilton product), not normalised.  a and b are read before r is written: r may be a or b
__device__ __forceinline__ void quat_mul(const double a[4], const double b[4], double r[4]) {
    const double ax = a[0], ay = a[1], az = a[2], aw = a[3], bx = b[0], by = b[1], bz = b[2], bw = b[3];
    r[3] = ((aw * bw - ax * bx) - ay * by) - az * bz;
    r[0] = ((aw * bx + ax * bw) + ay * bz) - az * by;
    r[1] = ((aw * by + ay * bw) + az * bx) - ax * bz;
    r[2] = ((aw * bz + az * bw) + ax * by) - ay * bx;
}

// VertexSE3Expmap::oplusImpl: estimate = SE3Quat::exp(x) * estimate (se3quat.h:223-257, :104-110); x = omega | upsilon; the
// estimate is t, q (two arrays that do not overlap)
__device__ __forceinline__ void se3_oplus(double t[3], double q[4], const double x[6]) {
    const double o0 = x[0], o1 = x[1], o2 = x[2];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double Om2[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Om2[r * 3 + c] = (Om[r * 3] * Om[c] + Om[r * 3 + 1] * Om[3 + c]) + Om[r * 3 + 2] * Om[6 + c];
    double a, b, c2;
    if (theta < 0.00001) { a = 1.0; b = 1.0; c2 = 1.0; }   // R = I + Omega + Omega^2, V = R
    else {
        const double s = sin(theta), co = cos(theta);
        a = s / theta; b = (1.0 - co) / (theta * theta); c2 = (theta - s) / (theta * theta * theta);
    }
    double R[9], V[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double id = (k == 0 || k == 4 || k == 8) ? 1.0 : 0.0;
        R[k] = (id + a * Om[k]) + b * Om2[k];
        V[k] = theta < 0.00001 ? R[k] : (id + b * Om[k]) + c2 * Om2[k];
    }
    double qe[4], te[3];
    quat_from_R(R, qe);
    normalize_rotation(qe);
#pragma unroll
    for (int r = 0; r < 3; r++) te[r] = (V[r * 3] * x[3] + V[r * 3 + 1] * x[4]) + V[r * 3 + 2] * x[5];
    double rt[3];
    quat_rotate(qe, t, rt);
    t[0] = te[0] + rt[0]; t[1] = te[1] + rt[1]; t[2] = te[2] + rt[2];
    quat_mul(qe, q, q);
    normalize_rotation(q);
}

// ------------------------------------------------------------------------------------
// g2o::Sim3 on orbg_sim3_t (q, t, s)
// Sim3::operator* (sim3.h:266-272): the quaternion product is not normalised
__device__ __forceinline__ orbg_sim3_t sim3_mul(const orbg_sim3_t &a, const orbg_sim3_t &b) {
    orbg_sim3_t r;
    quat_mul(a.q, b.q, r.q);
    double rt[3];
    quat_rotate(a.q, b.t, rt);
    r.t[0] = a.s * rt[0] + a.t[0]; r.t[1] = a.s * rt[1] + a.t[1]; r.t[2] = a.s * rt[2] + a.t[2];
    r.s = a.s * b.s;
    return r;
}
// Sim3::inverse (sim3.h:233-236): (r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
__device__ __forceinline__ orbg_sim3_t sim3_inverse(const orbg_sim3_t &a) {
    orbg_sim3_t r;
    r.q[0] = -a.q[0]; r.q[1] = -a.q[1]; r.q[2] = -a.q[2]; r.q[3] = a.q[3];
    const double k = -1. / a.s;
    const double v[3] = {k * a.t[0], k * a.t[1], k * a.t[2]};
    quat_rotate(r.q, v, r.t);
    r.s = 1. / a.s;
    return r;
}
__device__ __forceinline__ void sim3_map(const orbg_sim3_t &S, const double p[3], double r[3]) {   // sim3.h:144-146: s * (r * xyz) + t
    double v[3];
    quat_rotate(S.q, p, v);
    r[0] = S.s * v[0] + S.t[0]; r[1] = S.s * v[1] + S.t[1]; r[2] = S.s * v[2] + S.t[2];
}
// Sim3(const Vector7d &update) (sim3.h:70-142), update = omega | upsilon | sigma, with its four branches as written.  A numeric
// Jacobian's steps of 1e-9 always take the first (R = I + Omega + Omega^2, A = 1/2, B = 1/6, C = 1): no sin / cos there.
__device__ __forceinline__ orbg_sim3_t sim3_exp(const double u[7]) {
    const double o0 = u[0], o1 = u[1], o2 = u[2], sigma = u[6];
    const double theta = sqrt((o0 * o0 + o1 * o1) + o2 * o2);
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double Om2[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Om2[r * 3 + c] = (Om[r * 3] * Om[c] + Om[r * 3 + 1] * Om[3 + c]) + Om[r * 3 + 2] * Om[6 + c];
    orbg_sim3_t S;
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
    quat_from_R(R, S.q);
#pragma unroll
    for (int r = 0; r < 3; r++) S.t[r] = (W[r * 3] * u[3] + W[r * 3 + 1] * u[4]) + W[r * 3 + 2] * u[5];
    return S;
}

// ------------------------------------------------------------------------------------
// (H + lambda I) x = b, N square, by an unpivoted LDL^T in double; Hu: the N (N + 1) / 2 upper entries of H, row-major.  false when
// a pivot is not positive or not finite (LinearSolverDense: !isPositive()): then x = 0 and the caller leaves the estimate unchanged
// for that trial (tempChi = DBL_MAX rejects it), where g2o applies whatever x its solver still held before it restores the estimate.
// A zero row / column of H (the Sim3 vertex's row 6 with a fixed scale) is no failure: D = lambda there, x = 0 / lambda = 0.  Where
// Eigen's pivoted LDLT would decide differently (a singular H) the behaviour is not pinned.
template <int N>
__device__ __forceinline__ bool ldlt_solve(const double *Hu, const double *b, double lambda, double *x) {
    double A[N][N], L[N][N], D[N];
    int k = 0;
#pragma unroll
    for (int j = 0; j < N; j++)
#pragma unroll
        for (int l = j; l < N; l++, k++) { A[j][l] = Hu[k]; A[l][j] = Hu[k]; }
#pragma unroll
    for (int j = 0; j < N; j++) A[j][j] += lambda;
    bool ok = true;
#pragma unroll
    for (int j = 0; j < N; j++) {
        double d = A[j][j];
#pragma unroll
        for (int m = 0; m < j; m++) d -= (L[j][m] * L[j][m]) * D[m];
        if (!(d > 0.0) || !(d <= DBL_MAX)) ok = false;
        D[j] = d;
#pragma unroll
        for (int i = j + 1; i < N; i++) {
            double s = A[i][j];
#pragma unroll
            for (int m = 0; m < j; m++) s -= (L[i][m] * L[j][m]) * D[m];
            L[i][j] = s / d;
        }
    }
    double yv[N];
#pragma unroll
    for (int i = 0; i < N; i++) {
        double s = b[i];
#pragma unroll
        for (int m = 0; m < i; m++) s -= L[i][m] * yv[m];
        yv[i] = s;
    }
#pragma unroll
    for (int i = 0; i < N; i++) yv[i] = yv[i] / D[i];
#pragma unroll
    for (int i = N - 1; i >= 0; i--) {
        double s = yv[i];
#pragma unroll
        for (int m = i + 1; m < N; m++) s -= L[m][i] * x[m];
        x[i] = s;
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < N; i++) x[i] = 0.0;
    }
    return ok;
}
