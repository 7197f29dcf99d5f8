// orbx_lba.hip — Optimizer::LocalBundleAdjustment (reference: src/Optimizer.cc:453-780) and Optimizer::BundleAdjustment (:49-237):
// 6-DoF keyframe vertices (VertexSE3Expmap), 3-DoF map-point vertices (VertexSBAPointXYZ, always marginalised), one binary edge
// per observation (EdgeSE3ProjectXYZ, EdgeStereoSE3ProjectXYZ), Levenberg-Marquardt over the Schur complement.  A restatement of
// the reference and of the g2o classes it drives (types_six_dof_expmap, se3quat.h, base_binary_edge.hpp, block_solver.hpp,
// optimization_algorithm_levenberg, sparse_optimizer), double throughout with the reference's float narrowings; DESIGN.md
// section 6 has the list.  tests/lba_ref.py is the same arithmetic in numpy, statement for statement.
//
// The landmark block is block-diagonal 3x3, every Hpl block belongs to one edge, and the reduced system is 6 Nf square for Nf free
// keyframes (a few tens): dense and small.  The HOST drives the iterations and trials (lba_drive): it queues a handful of launches
// per linearisation and per trial on one stream and reads one small record (LbaRec) after each trial - one stream synchronisation,
// no device-wide one, and the stop flag is polled exactly where the reference reads it.  No cooperative launch, no grid barrier,
// no wait loop in a kernel, no floating-point atomics.  Every sum has one owner and a fixed order:
//   Hll / bl of a point        one thread: the point's active observations in ascending input index            (k_lba_point)
//   Hpp / bp of a free pose    one workgroup: the thread's edges ascending, wave butterfly, the waves in order  (k_lba_pose)
//   a Schur block (i1, i2)     one workgroup: the shared points in ascending point index, summed the same way   (k_lba_schur)
//   chi2, computeScale         per-workgroup partial sums, then one workgroup over the partials in order        (k_lba_*_reduce)
// so two runs give the same bytes.  The reduced system is factorised by ONE workgroup (k_lba_solve): LDL^T without pivoting, in
// LDS up to LBA_LDS_POSES free poses and in device memory past it - the same code through one pointer, hence the same bytes.
// A loop-closure-sized map (orbb_global_bundle_adjustment, orbb_optimize_blocked) takes the BLOCKED path between Dinv and the update:
// the Schur complement from the host-built list of co-observing pairs (k_gba_schur) and a dense LDL^T blocked over the grid in
// panels of GBA_PANEL_POSES poses (k_gba_diag / rows / trail, the substitutions likewise), every entry with k_lba_solve's operations
// in k_lba_solve's order.
#ifdef ORBX_LBA_HOST
// tests/cpp/lba_lockstep.cc compiles this file's kernels AND the driver for the host, one thread per workgroup, the workgroups
// of a launch one after the other (tests/cpp/hip_lockstep.h comes first): every sum then runs in ascending order, which is
// tests/lba_ref.py's order - the two must agree bit for bit (tests/test_lba_cpu.py).
#include "orbx_stage_plan.h"
#define LBA_THREADS 1
#define LBA_LANES 1
#else
#include "orbx_stage.h"
#define LBA_THREADS 256
#define LBA_LANES 64
#endif
#include <float.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "orbx_g2omath.h"

#define LBA_WAVES ((LBA_THREADS + LBA_LANES - 1) / LBA_LANES)
#define LBA_LDS_POSES 14    // free poses whose reduced system (6 * 14 = 84 square, 56448 B of doubles) is factorised in LDS, under the 64 KiB a launch gets unasked
#define LBA_ED 54           // doubles an edge's linearisation leaves: Hll 6 | bl 3 | Hpp 21 | bp 6 | W = Hpl 18
#define LBA_MAX_TRIALS 10   // g2o's maxTrialsAfterFailure
#define GBA_PANEL_POSES 8   // the blocked path (k_gba_*): poses of one panel of the blocked LDL^T, 6 * 8 = 48 columns; its diagonal block (18432 B) is factorised in LDS
#define GBA_NB (6 * GBA_PANEL_POSES)
#define GBA_TILE 64         // edge of a tile of the trailing update: 256 threads, a 4 x 4 micro-tile each
#define GBA_TS (GBA_TILE + 1)   // a staged strip's row stride in LDS: the odd stride spreads the transposing stores over the banks

struct LbaRec { double linChi, maxDiag, tmpChi, scale; int32_t ok, pad; };   // what the host reads after a linearisation (it == 0) and after every trial
struct LbaDev {
    int32_t K, P, E, nf;                  // keyframes, points, observations; free poses with an active edge this round (columns)
    const orbb_keyframe_t *kf; const orbb_point_t *pts; const orbb_observation_t *obs;
    const int32_t *ptStart, *ptEdges, *kfStart, *kfEdges;   // CSR by point and by keyframe, the edges of an owner in ascending input index
    const int32_t *col, *kfOfCol;         // per round: keyframe -> column (-1: fixed, or no active edge) and back
    int32_t *tab;                         // per round: [nf][P] the active edge of (column, point) or -1 (the dense path only)
    const int32_t *blk, *ca, *cb;         // the blocked path, per round: the pattern's blocks (i1, i2), i1 <= i2, sorted; a block's contributions (edge of i1, edge of i2)
    const long long *blkStart;            // ... in ascending point index, as a CSR over the blocks
    int32_t *bad;                         // the blocked path: a pivot of this trial was not > 0 or not finite
    double *pose[2], *pt[2];              // the estimates t[3] | q[4] (x y z w) per keyframe and xyz per point: current and trial, swapped by the host
    uint8_t *flag, *erase, *pact;         // edge at level 1; the final classification; point has an active edge
    double *chi2, *ed, *Hll, *bl, *Dinv, *db, *Hpp, *bp, *S, *xp, *partChi, *partScale;
    LbaRec *rec;
    float *outT, *outP; double *estKf, *estPt;
};
// block_sum, the quaternion functions and se3_oplus are orbx_g2omath.h's; part: LBA_WAVES * K doubles of LDS

// the estimates as the reference sets them (:527, :576): SE3Quat(R, t) of the widened float Tcw, the widened float position; every
// edge at level 0, no evaluation yet (an edge never evaluated reports chi2 = 0, where the reference reads an uninitialised error)
__global__ __launch_bounds__(LBA_THREADS) void k_lba_init(LbaDev D) {
    const int i = blockIdx.x * LBA_THREADS + threadIdx.x;
    if (i < D.K) {
        const float *Tf = D.kf[i].Tcw;
        double R[9], T[7];
#pragma unroll
        for (int r = 0; r < 3; r++) {
#pragma unroll
            for (int c = 0; c < 3; c++) R[r * 3 + c] = (double)Tf[r * 4 + c];
            T[r] = (double)Tf[r * 4 + 3];
        }
        quat_from_R(R, T + 3);
        normalize_rotation(T + 3);
#pragma unroll
        for (int k = 0; k < 7; k++) { D.pose[0][(size_t)i * 7 + k] = T[k]; D.pose[1][(size_t)i * 7 + k] = T[k]; }
    }
    if (i < D.P) {
        const orbb_point_t p = D.pts[i];
        const double X[3] = {(double)p.x, (double)p.y, (double)p.z};
#pragma unroll
        for (int k = 0; k < 3; k++) { D.pt[0][(size_t)i * 3 + k] = X[k]; D.pt[1][(size_t)i * 3 + k] = X[k]; }
        D.pact[i] = 0;
    }
    if (i < D.E) { D.flag[i] = 0; D.erase[i] = 0; D.chi2[i] = 0.0; }
}

// per round: the active edge of (column, point); tab was filled with -1
__global__ __launch_bounds__(LBA_THREADS) void k_lba_table(LbaDev D) {
    const int e = blockIdx.x * LBA_THREADS + threadIdx.x;
    if (e >= D.E || D.flag[e]) return;
    const orbb_observation_t o = D.obs[e];
    const int c = D.col[o.kf];
    if (c >= 0) D.tab[(size_t)c * D.P + o.pt] = e;
}

// One active edge per thread at estimate `c`: computeError, chi2, the Huber kernel; its rho[0] into the workgroup's partial sum.
// LIN: + linearizeOplus and constructQuadraticForm, the edge's own terms left in ed[k * E + e] for their owners to sum.  A monocular
// edge is the stereo one with a zero third row.
template <bool LIN>
__global__ __launch_bounds__(LBA_THREADS) void k_lba_edges(LbaDev D, int c, int robust, double dMono, double dStereo) {
    __shared__ double part[LBA_WAVES];
    const int e = blockIdx.x * LBA_THREADS + threadIdx.x;
    double a1[1] = {0.0};
    if (e < D.E && !D.flag[e]) {
        const orbb_observation_t o = D.obs[e];
        const orbb_keyframe_t *kf = D.kf + o.kf;
        const double fx = (double)kf->fx, fy = (double)kf->fy, cx = (double)kf->cx, cy = (double)kf->cy, bf = (double)kf->bf;
        const double *T = D.pose[c] + (size_t)o.kf * 7, *Xp = D.pt[c] + (size_t)o.pt * 3;
        const double q[4] = {T[3], T[4], T[5], T[6]}, Xw[3] = {Xp[0], Xp[1], Xp[2]};
        double X[3];
        quat_rotate(q, Xw, X);   // SE3Quat::map: _r * xyz + _t
        const double x = X[0] + T[0], y = X[1] + T[1], z = X[2] + T[2];
        const bool mono = o.ur < 0.f;
        double e0, e1, e2;
        if (mono) {   // project2d, then * f + c, in double (types_six_dof_expmap.cpp:141-147)
            e0 = (double)o.u - ((x / z) * fx + cx);
            e1 = (double)o.v - ((y / z) * fy + cy);
            e2 = 0.0;
        } else {      // cam_project(trans_xyz, const float &bf) (:150-157): invz AND bf are float there, so bf * invz is a float product
            const float izf = (float)(1.0 / z);
            const double iz = (double)izf;
            const double pu = (x * iz) * fx + cx;
            e0 = (double)o.u - pu;
            e1 = (double)o.v - ((y * iz) * fy + cy);
            e2 = (double)o.ur - (pu - (double)(kf->bf * izf));
        }
        const double is2 = (double)o.inv_sigma2;
        const double oe0 = is2 * e0, oe1 = is2 * e1, oe2 = is2 * e2;
        const double chi2 = (e0 * oe0 + e1 * oe1) + e2 * oe2;
        const double delta = mono ? dMono : dStereo;
        const double dsqr = delta * delta;
        double rho0 = chi2, w = 1.0;
        if (robust && !(chi2 <= dsqr)) {
            const double s = sqrt(chi2);
            rho0 = (2.0 * s) * delta - dsqr;
            w = delta / s;
        }
        D.chi2[e] = chi2;
        a1[0] = rho0;
        if (LIN) {
            double R[9], A[3][3], B[3][6];
            quat_to_R(q, R);
            const double z_2 = z * z;
            if (mono) {   // _jacobianOplusXi = -1./z * tmp * R, tmp = [fx 0 -x/z*fx; 0 fy -y/z*fy] (:115-124)
                const double s = -1. / z;
                const double t0[3] = {s * fx, s * 0.0, s * (((-x) / z) * fx)}, t1[3] = {s * 0.0, s * fy, s * (((-y) / z) * fy)};
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    A[0][k] = (t0[0] * R[k] + t0[1] * R[3 + k]) + t0[2] * R[6 + k];
                    A[1][k] = (t1[0] * R[k] + t1[1] * R[3 + k]) + t1[2] * R[6 + k];
                    A[2][k] = 0.0;
                }
            } else {      // entry by entry (:202-212)
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    A[0][k] = ((-fx) * R[k]) / z + ((fx * x) * R[6 + k]) / z_2;
                    A[1][k] = ((-fy) * R[3 + k]) / z + ((fy * y) * R[6 + k]) / z_2;
                    A[2][k] = A[0][k] - (bf * R[6 + k]) / z_2;
                }
            }
            B[0][0] = ((x * y) / z_2) * fx;            // _jacobianOplusXj (:126-138, :214-233)
            B[0][1] = -(1 + ((x * x) / z_2)) * fx;
            B[0][2] = (y / z) * fx;
            B[0][3] = (-1. / z) * fx;
            B[0][4] = 0.0;
            B[0][5] = (x / z_2) * fx;
            B[1][0] = (1 + (y * y) / z_2) * fy;
            B[1][1] = (((-x) * y) / z_2) * fy;
            B[1][2] = ((-x) / z) * fy;
            B[1][3] = 0.0;
            B[1][4] = (-1. / z) * fy;
            B[1][5] = (y / z_2) * fy;
            if (mono) {
#pragma unroll
                for (int j = 0; j < 6; j++) B[2][j] = 0.0;
            } else {
                B[2][0] = B[0][0] - (bf * y) / z_2;
                B[2][1] = B[0][1] + (bf * x) / z_2;
                B[2][2] = B[0][2];
                B[2][3] = B[0][3];
                B[2][4] = 0.0;
                B[2][5] = B[0][5] - bf / z_2;
            }
            const double wo = w * is2;   // robustInformation: rho[1] * information; omega_r = -(information * error) * rho[1]
            double *ed = D.ed + e;
            const size_t E = (size_t)D.E;
            int k = 0;
#pragma unroll
            for (int j = 0; j < 3; j++)
#pragma unroll
                for (int l = j; l < 3; l++, k++) ed[k * E] = ((A[0][j] * wo) * A[0][l] + (A[1][j] * wo) * A[1][l]) + (A[2][j] * wo) * A[2][l];
#pragma unroll
            for (int j = 0; j < 3; j++, k++) ed[k * E] = -(w * ((A[0][j] * oe0 + A[1][j] * oe1) + A[2][j] * oe2));
#pragma unroll
            for (int j = 0; j < 6; j++)
#pragma unroll
                for (int l = j; l < 6; l++, k++) ed[k * E] = ((B[0][j] * wo) * B[0][l] + (B[1][j] * wo) * B[1][l]) + (B[2][j] * wo) * B[2][l];
#pragma unroll
            for (int j = 0; j < 6; j++, k++) ed[k * E] = -(w * ((B[0][j] * oe0 + B[1][j] * oe1) + B[2][j] * oe2));
#pragma unroll
            for (int j = 0; j < 6; j++)       // W = Hpl = B^T (rho[1] Omega) A, 6 x 3
#pragma unroll
                for (int l = 0; l < 3; l++, k++) ed[k * E] = ((B[0][j] * wo) * A[0][l] + (B[1][j] * wo) * A[1][l]) + (B[2][j] * wo) * A[2][l];
        }
    }
    block_sum<LBA_LANES, LBA_WAVES>(a1, part);
    if (threadIdx.x == 0) D.partChi[blockIdx.x] = a1[0];
}

// Hll and bl of a point: its active observations in ascending input index.  A point without one has left the problem.
__global__ __launch_bounds__(LBA_THREADS) void k_lba_point(LbaDev D) {
    const int p = blockIdx.x * LBA_THREADS + threadIdx.x;
    if (p >= D.P) return;
    double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int n = 0;
    const size_t E = (size_t)D.E;
    for (int i = D.ptStart[p]; i < D.ptStart[p + 1]; i++) {
        const int e = D.ptEdges[i];
        if (D.flag[e]) continue;
        n++;
#pragma unroll
        for (int k = 0; k < 9; k++) acc[k] += D.ed[k * E + e];
    }
    D.pact[p] = n > 0;
#pragma unroll
    for (int k = 0; k < 6; k++) D.Hll[(size_t)p * 6 + k] = acc[k];
#pragma unroll
    for (int k = 0; k < 3; k++) D.bl[(size_t)p * 3 + k] = acc[6 + k];
}

// Hpp and bp of a free pose (column blockIdx.x): one workgroup
__global__ __launch_bounds__(LBA_THREADS) void k_lba_pose(LbaDev D) {
    __shared__ double part[LBA_WAVES * 27];
    const int c = blockIdx.x, kf = D.kfOfCol[c];
    double acc[27];
#pragma unroll
    for (int k = 0; k < 27; k++) acc[k] = 0.0;
    const size_t E = (size_t)D.E;
    for (int i = D.kfStart[kf] + (int)threadIdx.x; i < D.kfStart[kf + 1]; i += LBA_THREADS) {
        const int e = D.kfEdges[i];
        if (D.flag[e]) continue;
#pragma unroll
        for (int k = 0; k < 27; k++) acc[k] += D.ed[(9 + k) * E + e];
    }
    block_sum<LBA_LANES, LBA_WAVES>(acc, part);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 21; k++) D.Hpp[(size_t)c * 21 + k] = acc[k];
#pragma unroll
        for (int k = 0; k < 6; k++) D.bp[(size_t)c * 6 + k] = acc[21 + k];
    }
}

// after a linearisation: activeRobustChi2 from the partial sums, and computeLambdaInit's max |diagonal| over the active vertices.
// computeLambdaInit (optimization_algorithm_levenberg.cpp:171-178) walks the diagonal - the poses' entries, then the points' - with
// maxDiagonal = std::max(fabs(h), maxDiagonal), which keeps its FIRST argument unless that is the smaller one: a NaN entry replaces
// the running maximum, and the entry after it replaces the NaN.  So the result is the maximum over the entries after the last NaN,
// and NaN when the last entry is one.  Without a NaN that is the plain maximum (from 0).
__global__ __launch_bounds__(LBA_THREADS) void k_lba_lin_reduce(LbaDev D, int nbE) {
    __shared__ double part[LBA_WAVES];
    __shared__ double mx[LBA_THREADS];
    __shared__ long long at[LBA_THREADS];
    const int dp[6] = {0, 6, 11, 15, 18, 20}, dl[3] = {0, 3, 5};
    const int tid = threadIdx.x;
    double a1[1] = {0.0}, md = 0.0;
    for (int i = tid; i < nbE; i += LBA_THREADS) a1[0] += D.partChi[i];
    block_sum<LBA_LANES, LBA_WAVES>(a1, part);
    long long last = -1;               // the last NaN's place in computeLambdaInit's walk
    for (int i = tid; i < D.nf; i += LBA_THREADS)
        for (int j = 0; j < 6; j++) {
            const double h = D.Hpp[(size_t)i * 21 + dp[j]];
            if (h != h) last = (long long)i * 6 + j;
            md = fmax(fabs(h), md);    // fmax drops a NaN: the plain maximum, which is the answer when there is none
        }
    for (int i = tid; i < D.P; i += LBA_THREADS) {
        if (!D.pact[i]) continue;
        for (int l = 0; l < 3; l++) {
            const double h = D.Hll[(size_t)i * 6 + dl[l]];
            if (h != h) last = (long long)D.nf * 6 + (long long)i * 3 + l;
            md = fmax(fabs(h), md);
        }
    }
    at[tid] = last; mx[tid] = md;
    __syncthreads();
    for (int s = LBA_THREADS / 2; s > 0; s >>= 1) {   // maxima of numbers: any order gives the same value
        if (tid < s) { at[tid] = at[tid + s] > at[tid] ? at[tid + s] : at[tid]; mx[tid] = fmax(mx[tid + s], mx[tid]); }
        __syncthreads();
    }
    last = at[0];
    if (last >= 0) {                   // uniform over the workgroup: a NaN on the diagonal, so only the entries after the last one count
        md = -1.0;                     // -1: no such entry yet (every |h| is at least 0)
        for (int i = tid; i < D.nf; i += LBA_THREADS)
            for (int j = 0; j < 6; j++)
                if ((long long)i * 6 + j > last) md = fmax(fabs(D.Hpp[(size_t)i * 21 + dp[j]]), md);
        for (int i = tid; i < D.P; i += LBA_THREADS) {
            if (!D.pact[i]) continue;
            for (int l = 0; l < 3; l++)
                if ((long long)D.nf * 6 + (long long)i * 3 + l > last) md = fmax(fabs(D.Hll[(size_t)i * 6 + dl[l]]), md);
        }
        mx[tid] = md;                  // nobody reads mx between the loop's last barrier and the next one
        __syncthreads();
        for (int s = LBA_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) mx[tid] = fmax(mx[tid + s], mx[tid]);
            __syncthreads();
        }
    }
    if (tid == 0) {
        D.rec->linChi = a1[0];
        D.rec->maxDiag = mx[0] >= 0.0 ? mx[0] : NAN;
    }
}

// a trial: Dinv = (Hll + lambda I)^-1 in closed form (cofactors over the determinant) and Dinv * bl, per active point
__global__ __launch_bounds__(LBA_THREADS) void k_lba_dinv(LbaDev D, double lambda) {
    const int p = blockIdx.x * LBA_THREADS + threadIdx.x;
    if (p >= D.P || !D.pact[p]) return;
    const double *H = D.Hll + (size_t)p * 6, *b = D.bl + (size_t)p * 3;
    const double a00 = H[0] + lambda, a01 = H[1], a02 = H[2], a11 = H[3] + lambda, a12 = H[4], a22 = H[5] + lambda;
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double id = 1.0 / det;
    const double i00 = c00 * id, i01 = c01 * id, i02 = c02 * id, i11 = c11 * id, i12 = c12 * id, i22 = c22 * id;
    double *Di = D.Dinv + (size_t)p * 6, *db = D.db + (size_t)p * 3;
    Di[0] = i00; Di[1] = i01; Di[2] = i02; Di[3] = i11; Di[4] = i12; Di[5] = i22;
    db[0] = (i00 * b[0] + i01 * b[1]) + i02 * b[2];
    db[1] = (i01 * b[0] + i11 * b[1]) + i12 * b[2];
    db[2] = (i02 * b[0] + i12 * b[1]) + i22 * b[2];
}

// Block (i1, i2), i1 <= i2, of Hschur = (Hpp + lambda I) - sum_p W Dinv W^T over the points both poses observe, in ascending point
// index; the diagonal blocks also form bschur = bp - sum_p W Dinv bl.  Only the lower triangle of S is written (row >= column):
// block (i1, i2) lands transposed at rows 6 i2.., columns 6 i1...
__global__ __launch_bounds__(LBA_THREADS) void k_lba_schur(LbaDev D, double lambda) {
    __shared__ double part[LBA_WAVES * 42];
    const int nf = D.nf, i1 = blockIdx.x / nf, i2 = blockIdx.x % nf;
    if (i2 < i1) return;   // uniform over the workgroup
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; k++) acc[k] = 0.0;
    const size_t E = (size_t)D.E;
    const int32_t *t1 = D.tab + (size_t)i1 * D.P, *t2 = D.tab + (size_t)i2 * D.P;
    for (int p = threadIdx.x; p < D.P; p += LBA_THREADS) {
        const int ea = t1[p], eb = t2[p];
        if (ea < 0 || eb < 0) continue;
        const double *Dp = D.Dinv + (size_t)p * 6;
        const double Di[3][3] = {{Dp[0], Dp[1], Dp[2]}, {Dp[1], Dp[3], Dp[4]}, {Dp[2], Dp[4], Dp[5]}};
        double Y[6][3], W2[6][3];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double w0 = D.ed[(36 + j * 3) * E + ea], w1 = D.ed[(37 + j * 3) * E + ea], w2 = D.ed[(38 + j * 3) * E + ea];
#pragma unroll
            for (int l = 0; l < 3; l++) {
                Y[j][l] = (w0 * Di[0][l] + w1 * Di[1][l]) + w2 * Di[2][l];
                W2[j][l] = D.ed[(36 + j * 3 + l) * E + eb];
            }
            if (i1 == i2) {
                const double *db = D.db + (size_t)p * 3;
                acc[36 + j] += (w0 * db[0] + w1 * db[1]) + w2 * db[2];
            }
        }
#pragma unroll
        for (int j = 0; j < 6; j++)
#pragma unroll
            for (int l = 0; l < 6; l++) acc[j * 6 + l] += (Y[j][0] * W2[l][0] + Y[j][1] * W2[l][1]) + Y[j][2] * W2[l][2];
    }
    block_sum<LBA_LANES, LBA_WAVES>(acc, part);
    if (threadIdx.x == 0) {
        const size_t n = (size_t)nf * 6;
        if (i1 == i2) {
            const double *H = D.Hpp + (size_t)i1 * 21;
            int k = 0;
            for (int j = 0; j < 6; j++)
                for (int l = j; l < 6; l++, k++)   // H's upper entry (j, l) is the lower entry (l, j)
                    D.S[(size_t)(6 * i1 + l) * n + 6 * i1 + j] = (j == l ? H[k] + lambda : H[k]) - acc[l * 6 + j];
            for (int j = 0; j < 6; j++) D.xp[6 * i1 + j] = D.bp[(size_t)i1 * 6 + j] - acc[36 + j];
        } else {
            for (int j = 0; j < 6; j++)
                for (int l = 0; l < 6; l++) D.S[(size_t)(6 * i2 + l) * n + 6 * i1 + j] = 0.0 - acc[j * 6 + l];
        }
    }
}

// Hschur xp = bschur (xp holds bschur on entry): right-looking LDL^T without pivoting on the lower triangle, then the two
// substitutions column by column, so that every entry's updates arrive in one fixed order whatever the number of threads.  A zero,
// negative or non-finite pivot: ok = 0 and xp = 0 (LinearSolver: !ok -> the trial's tempChi is DBL_MAX).  nf == 0: nothing to solve.
__global__ __launch_bounds__(LBA_THREADS) void k_lba_solve(LbaDev D, int inLds) {
    extern __shared__ __align__(16) uint8_t lba_lds[];
    __shared__ int bad;
    const int n = D.nf * 6, tid = threadIdx.x;
    double *A = inLds ? (double *)lba_lds : D.S, *v = D.xp;
    if (tid == 0) bad = 0;
    if (inLds)
        for (int i = tid; i < n * n; i += LBA_THREADS)
            if (i / n >= i % n) A[i] = D.S[i];
    __syncthreads();
    for (int m = 0; m < n; m++) {
        const double d = A[(size_t)m * n + m];
        if (tid == 0 && (!(d > 0.0) || !(d <= DBL_MAX))) bad = 1;
        __syncthreads();   // everyone has read the pivot's column as the last step left it
        for (int i = m + 1 + tid; i < n; i += LBA_THREADS) A[(size_t)i * n + m] = A[(size_t)i * n + m] / d;
        __syncthreads();
        const int r = n - m - 1;
        for (int t = tid; t < r * r; t += LBA_THREADS) {
            const int i = m + 1 + t / r, j = m + 1 + t % r;
            if (j <= i) A[(size_t)i * n + j] -= (A[(size_t)i * n + m] * A[(size_t)j * n + m]) * d;
        }
        __syncthreads();
    }
    for (int m = 0; m < n; m++) {          // L y = b
        const double ym = v[m];
        for (int i = m + 1 + tid; i < n; i += LBA_THREADS) v[i] -= A[(size_t)i * n + m] * ym;
        __syncthreads();
    }
    for (int i = tid; i < n; i += LBA_THREADS) v[i] = v[i] / A[(size_t)i * n + i];
    __syncthreads();
    for (int m = n - 1; m >= 0; m--) {     // L^T x = y
        const double xm = v[m];
        for (int i = tid; i < m; i += LBA_THREADS) v[i] -= A[(size_t)m * n + i] * xm;
        __syncthreads();
    }
    if (bad)
        for (int i = tid; i < n; i += LBA_THREADS) v[i] = 0.0;
    if (tid == 0) D.rec->ok = bad ? 0 : 1;
}

// ------------------------------------------------------------------------------------
// The blocked reduced-system path (orbb_optimize_blocked, orbb_global_bundle_adjustment): k_gba_schur and the k_gba_* factorisation
// stand where k_lba_table, k_lba_schur and k_lba_solve stand on the dense path; everything before Dinv and from k_lba_update on is
// shared.  The contract: every entry of S, of the factor and of the solution receives exactly the operations k_lba_solve applies to
// it, in the same order - updates x -= (L_im * L_jm) * d_m in ascending m, then the division by the pivot; forward substitution in
// ascending m, backward in descending m; no contraction.  Blocking changes which thread does an operation, never its rounding, so
// one thread per workgroup gives tests/lba_ref.py's bytes and the factor does not depend on the launch shape.  Hence no matrix
// cores and no skipping of structurally zero tiles (-0.0 - (-0.0) changes a sign bit).
//
// Block `blockIdx.x` of the pattern, one WORKGROUP its owner: the block's contributions W_a Dinv W_b^T in ascending point index,
// the thread's terms ascending, wave butterfly, the waves in order - k_lba_schur's sum over a list instead of a [nf][P] table, and
// its inner expressions.  S was cleared on the stream: a block outside the pattern is +0.0, which is what k_lba_schur writes there.
__global__ __launch_bounds__(LBA_THREADS) void k_gba_schur(LbaDev D, double lambda) {
    __shared__ double part[LBA_WAVES * 42];
    const int b = blockIdx.x, nf = D.nf, i1 = D.blk[2 * b], i2 = D.blk[2 * b + 1];
    double acc[42];
#pragma unroll
    for (int k = 0; k < 42; k++) acc[k] = 0.0;
    const size_t E = (size_t)D.E;
    const long long t1 = D.blkStart[b + 1];
    for (long long t = D.blkStart[b] + (long long)threadIdx.x; t < t1; t += LBA_THREADS) {
        const int ea = D.ca[t], eb = D.cb[t];
        const size_t p = (size_t)D.obs[ea].pt;
        const double *Dp = D.Dinv + p * 6;
        const double Di[3][3] = {{Dp[0], Dp[1], Dp[2]}, {Dp[1], Dp[3], Dp[4]}, {Dp[2], Dp[4], Dp[5]}};
        double Y[6][3], W2[6][3];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            const double w0 = D.ed[(36 + j * 3) * E + ea], w1 = D.ed[(37 + j * 3) * E + ea], w2 = D.ed[(38 + j * 3) * E + ea];
#pragma unroll
            for (int l = 0; l < 3; l++) {
                Y[j][l] = (w0 * Di[0][l] + w1 * Di[1][l]) + w2 * Di[2][l];
                W2[j][l] = D.ed[(36 + j * 3 + l) * E + eb];
            }
            if (i1 == i2) {
                const double *db = D.db + p * 3;
                acc[36 + j] += (w0 * db[0] + w1 * db[1]) + w2 * db[2];
            }
        }
#pragma unroll
        for (int j = 0; j < 6; j++)
#pragma unroll
            for (int l = 0; l < 6; l++) acc[j * 6 + l] += (Y[j][0] * W2[l][0] + Y[j][1] * W2[l][1]) + Y[j][2] * W2[l][2];
    }
    block_sum<LBA_LANES, LBA_WAVES>(acc, part);
    if (threadIdx.x == 0) {
        const size_t n = (size_t)nf * 6;
        if (i1 == i2) {
            const double *H = D.Hpp + (size_t)i1 * 21;
            int k = 0;
            for (int j = 0; j < 6; j++)
                for (int l = j; l < 6; l++, k++)
                    D.S[(size_t)(6 * i1 + l) * n + 6 * i1 + j] = (j == l ? H[k] + lambda : H[k]) - acc[l * 6 + j];
            for (int j = 0; j < 6; j++) D.xp[6 * i1 + j] = D.bp[(size_t)i1 * 6 + j] - acc[36 + j];
        } else {
            for (int j = 0; j < 6; j++)
                for (int l = 0; l < 6; l++) D.S[(size_t)(6 * i2 + l) * n + 6 * i1 + j] = 0.0 - acc[j * 6 + l];
        }
    }
}

// A panel is the columns [c0, c0 + w) of S, w = GBA_NB but for the last.  Its launches: k_gba_diag (one workgroup), and where rows
// lie below it k_gba_rows (one thread per row) and k_gba_trail (one workgroup per 64 x 64 tile of the trailing lower triangle).
//
// The panel's diagonal block in LDS: k_lba_solve's elimination on w columns - every update from the columns left of c0 has
// arrived through k_gba_trail in ascending m - and the forward substitution's steps inside the block.  The pivot is judged at the
// moment it is used, by k_lba_solve's rule; the verdict outlives the launch in D.bad.
__global__ __launch_bounds__(LBA_THREADS) void k_gba_diag(LbaDev D, int n, int c0, int w) {
    __shared__ double A[GBA_NB * GBA_NB];
    const int tid = threadIdx.x;
    double *v = D.xp + c0;
    for (int t = tid; t < w * w; t += LBA_THREADS) {
        const int i = t / w, j = t % w;
        if (j <= i) A[i * GBA_NB + j] = D.S[(size_t)(c0 + i) * n + c0 + j];
    }
    __syncthreads();
    for (int m = 0; m < w; m++) {
        const double d = A[m * GBA_NB + m];
        if (tid == 0 && (!(d > 0.0) || !(d <= DBL_MAX))) *D.bad = 1;
        __syncthreads();
        for (int i = m + 1 + tid; i < w; i += LBA_THREADS) A[i * GBA_NB + m] = A[i * GBA_NB + m] / d;
        __syncthreads();
        const int r = w - m - 1;
        for (int t = tid; t < r * r; t += LBA_THREADS) {
            const int i = m + 1 + t / r, j = m + 1 + t % r;
            if (j <= i) A[i * GBA_NB + j] -= (A[i * GBA_NB + m] * A[j * GBA_NB + m]) * d;
        }
        __syncthreads();
    }
    for (int m = 0; m < w; m++) {          // L y = b inside the block
        const double ym = v[m];
        for (int i = m + 1 + tid; i < w; i += LBA_THREADS) v[i] -= A[i * GBA_NB + m] * ym;
        __syncthreads();
    }
    for (int t = tid; t < w * w; t += LBA_THREADS) {
        const int i = t / w, j = t % w;
        if (j <= i) D.S[(size_t)(c0 + i) * n + c0 + j] = A[i * GBA_NB + j];
    }
}

// The rows below a full panel, one thread per row i >= c0 + GBA_NB with the row's 48 entries in registers: column m is divided by
// its pivot, then entry j > m takes (L_im * L_jm) * d_m - ascending m per entry, the division last.  Then the row's share of the
// forward substitution, v[i] -= L_im * y_m over the panel in ascending m (y of the panel is final: k_gba_diag ran before).
__global__ __launch_bounds__(LBA_THREADS) void k_gba_rows(LbaDev D, int n, int c0) {
    __shared__ double Ld[GBA_NB * GBA_NB];
    __shared__ double dd[GBA_NB], yy[GBA_NB];
    const int tid = threadIdx.x;
    for (int t = tid; t < GBA_NB * GBA_NB; t += LBA_THREADS) Ld[t] = D.S[(size_t)(c0 + t / GBA_NB) * n + c0 + t % GBA_NB];
    for (int t = tid; t < GBA_NB; t += LBA_THREADS) { dd[t] = D.S[(size_t)(c0 + t) * n + c0 + t]; yy[t] = D.xp[c0 + t]; }
    __syncthreads();
    const int i = c0 + GBA_NB + (int)blockIdx.x * LBA_THREADS + tid;
    if (i >= n) return;
    double *row = D.S + (size_t)i * n + c0;
    double x[GBA_NB];
#pragma unroll
    for (int m = 0; m < GBA_NB; m++) x[m] = row[m];
#pragma unroll
    for (int m = 0; m < GBA_NB; m++) {
        const double d = dd[m];
        x[m] = x[m] / d;
#pragma unroll
        for (int j = m + 1; j < GBA_NB; j++) x[j] -= (x[m] * Ld[j * GBA_NB + m]) * d;
    }
    double vi = D.xp[i];
#pragma unroll
    for (int m = 0; m < GBA_NB; m++) { row[m] = x[m]; vi -= x[m] * yy[m]; }
    D.xp[i] = vi;
}

// Tile `blockIdx.x` of the lower triangle right of and below a full panel, tiles counted row by row: entry (i, j), j <= i, takes
// (L_im * L_jm) * d_m for the panel's m in ascending order.  The two strips of the panel - the tile's rows and the rows that are
// its columns - are staged transposed in LDS, [m][row]; a thread holds a 4 x 4 micro-tile.  Every tile is updated whatever it
// holds: a zero tile is not skipped.
__global__ __launch_bounds__(LBA_THREADS) void k_gba_trail(LbaDev D, int n, int c0) {
    __shared__ double Lr[GBA_NB * GBA_TS], Lc[GBA_NB * GBA_TS];
    __shared__ double dd[GBA_NB];
    const int tid = threadIdx.x, c1 = c0 + GBA_NB, t = blockIdx.x;
    int I = (int)((sqrt(8.0 * (double)t + 1.0) - 1.0) * 0.5);
    while (I * (I + 1) / 2 > t) I--;
    while ((I + 1) * (I + 2) / 2 <= t) I++;
    const int J = t - I * (I + 1) / 2, r0 = c1 + I * GBA_TILE, q0 = c1 + J * GBA_TILE;
    for (int s = tid; s < GBA_NB * GBA_TILE; s += LBA_THREADS) {
        const int m = s % GBA_NB, r = s / GBA_NB;
        Lr[m * GBA_TS + r] = r0 + r < n ? D.S[(size_t)(r0 + r) * n + c0 + m] : 0.0;
        Lc[m * GBA_TS + r] = q0 + r < n ? D.S[(size_t)(q0 + r) * n + c0 + m] : 0.0;
    }
    for (int s = tid; s < GBA_NB; s += LBA_THREADS) dd[s] = D.S[(size_t)(c0 + s) * n + c0 + s];
    __syncthreads();
    for (int mt = tid; mt < (GBA_TILE / 4) * (GBA_TILE / 4); mt += LBA_THREADS) {
        const int ty = mt / (GBA_TILE / 4), tx = mt % (GBA_TILE / 4), i0 = r0 + ty * 4, j0 = q0 + tx * 4;
        if (i0 >= n || j0 > i0 + 3) continue;   // below the matrix, or wholly above the diagonal
        double acc[4][4];
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[r][c] = (i0 + r < n && j0 + c <= i0 + r) ? D.S[(size_t)(i0 + r) * n + j0 + c] : 0.0;
#pragma unroll 4
        for (int m = 0; m < GBA_NB; m++) {
            const double d = dd[m];
            double a[4], b[4];
#pragma unroll
            for (int r = 0; r < 4; r++) { a[r] = Lr[m * GBA_TS + ty * 4 + r]; b[r] = Lc[m * GBA_TS + tx * 4 + r]; }
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[r][c] -= (a[r] * b[c]) * d;
        }
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++)
                if (i0 + r < n && j0 + c <= i0 + r) D.S[(size_t)(i0 + r) * n + j0 + c] = acc[r][c];
    }
}

// y / D, before any backward step
__global__ __launch_bounds__(LBA_THREADS) void k_gba_scale(LbaDev D, int n) {
    const int i = blockIdx.x * LBA_THREADS + threadIdx.x;
    if (i < n) D.xp[i] = D.xp[i] / D.S[(size_t)i * n + i];
}

// L^T x = y, the panels from the last to the first: inside the panel's block in descending m (one workgroup), then every entry left
// of the panel takes the panel's m in descending order (k_gba_back_rows, one thread per entry) - descending m per entry overall
__global__ __launch_bounds__(LBA_THREADS) void k_gba_back_diag(LbaDev D, int n, int c0, int w) {
    const int tid = threadIdx.x;
    double *v = D.xp + c0;
    for (int m = w - 1; m >= 0; m--) {
        const double xm = v[m];
        for (int i = tid; i < m; i += LBA_THREADS) v[i] -= D.S[(size_t)(c0 + m) * n + c0 + i] * xm;
        __syncthreads();
    }
}
__global__ __launch_bounds__(LBA_THREADS) void k_gba_back_rows(LbaDev D, int n, int c0, int w) {
    const int i = blockIdx.x * LBA_THREADS + threadIdx.x;
    if (i >= c0) return;
    double vi = D.xp[i];
    for (int m = c0 + w - 1; m >= c0; m--) vi -= D.S[(size_t)m * n + i] * D.xp[m];
    D.xp[i] = vi;
}

// k_lba_solve's end: after a bad pivot x = 0 and ok = 0.  n == 0: one workgroup, ok = 1.
__global__ __launch_bounds__(LBA_THREADS) void k_gba_finish(LbaDev D, int n) {
    const int i = blockIdx.x * LBA_THREADS + threadIdx.x, bad = *D.bad;
    if (bad && i < n) D.xp[i] = 0.0;
    if (i == 0) D.rec->ok = bad ? 0 : 1;
}

// The trial estimates from the current ones: workgroups [0, nbK) take the keyframes (exp(xp) * T for a column), the rest the points
// (xl = Dinv (bl - W^T xp) over the point's active edges in ascending input index, then +=).  A vertex outside the problem, and every
// vertex after a failed solve, is copied.  Each workgroup leaves its share of computeScale: sum x (lambda x + b).
// After a failed solve g2o's x is what the call before left there (block_solver.hpp:447-457 returns before writing it; solver.cpp:54
// allocates it without clearing), so the first failure reads memory nobody wrote.  Here x is zero then, and computeScale still runs
// over every entry as :185-187 does: 0 * (lambda * 0 + b) is NaN where b or lambda is not finite, and the trial is rejected.
__global__ __launch_bounds__(LBA_THREADS) void k_lba_update(LbaDev D, int c, double lambda, int nbK) {
    __shared__ double part[LBA_WAVES];
    const int ok = D.rec->ok;
    double a1[1] = {0.0};
    if ((int)blockIdx.x < nbK) {
        const int k = blockIdx.x * LBA_THREADS + threadIdx.x;
        if (k < D.K) {
            double T[7];
#pragma unroll
            for (int j = 0; j < 7; j++) T[j] = D.pose[c][(size_t)k * 7 + j];
            const int cl = D.col[k];
            if (cl >= 0) {
                double x[6], s = 0.0;
#pragma unroll
                for (int j = 0; j < 6; j++) x[j] = D.xp[cl * 6 + j];   // zero after a failed solve
#pragma unroll
                for (int j = 0; j < 6; j++) s += x[j] * (lambda * x[j] + D.bp[(size_t)cl * 6 + j]);
                a1[0] = s;
                if (ok) se3_oplus(T, T + 3, x);
            }
#pragma unroll
            for (int j = 0; j < 7; j++) D.pose[c ^ 1][(size_t)k * 7 + j] = T[j];
        }
    } else {
        const int p = ((int)blockIdx.x - nbK) * LBA_THREADS + threadIdx.x;
        if (p < D.P) {
            double X[3] = {D.pt[c][(size_t)p * 3], D.pt[c][(size_t)p * 3 + 1], D.pt[c][(size_t)p * 3 + 2]};
            if (D.pact[p]) {
                const double *b = D.bl + (size_t)p * 3, *Dp = D.Dinv + (size_t)p * 6;
                double cl[3] = {b[0], b[1], b[2]};
                const size_t E = (size_t)D.E;
                for (int i = D.ptStart[p]; ok && i < D.ptStart[p + 1]; i++) {
                    const int e = D.ptEdges[i];
                    if (D.flag[e]) continue;
                    const int cc = D.col[D.obs[e].kf];
                    if (cc < 0) continue;
                    const double *x = D.xp + cc * 6;
#pragma unroll
                    for (int l = 0; l < 3; l++) {
                        double t = 0.0;
#pragma unroll
                        for (int j = 0; j < 6; j++) t += D.ed[(36 + j * 3 + l) * E + e] * x[j];
                        cl[l] -= t;
                    }
                }
                double xl[3] = {(Dp[0] * cl[0] + Dp[1] * cl[1]) + Dp[2] * cl[2], (Dp[1] * cl[0] + Dp[3] * cl[1]) + Dp[4] * cl[2],
                                (Dp[2] * cl[0] + Dp[4] * cl[1]) + Dp[5] * cl[2]};
                if (!ok) xl[0] = xl[1] = xl[2] = 0.0;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 3; l++) { s += xl[l] * (lambda * xl[l] + b[l]); if (ok) X[l] += xl[l]; }
                a1[0] = s;
            }
#pragma unroll
            for (int l = 0; l < 3; l++) D.pt[c ^ 1][(size_t)p * 3 + l] = X[l];
        }
    }
    block_sum<LBA_LANES, LBA_WAVES>(a1, part);
    if (threadIdx.x == 0) D.partScale[blockIdx.x] = a1[0];
}

// after a trial: the trial's activeRobustChi2 and computeScale from the partial sums
__global__ __launch_bounds__(LBA_THREADS) void k_lba_trial_reduce(LbaDev D, int nbE, int nbS) {
    __shared__ double part[2][LBA_WAVES];
    double a1[1] = {0.0}, a2[1] = {0.0};
    for (int i = threadIdx.x; i < nbE; i += LBA_THREADS) a1[0] += D.partChi[i];
    for (int i = threadIdx.x; i < nbS; i += LBA_THREADS) a2[0] += D.partScale[i];
    block_sum<LBA_LANES, LBA_WAVES>(a1, part[0]);
    block_sum<LBA_LANES, LBA_WAVES>(a2, part[1]);
    if (threadIdx.x == 0) { D.rec->tmpChi = a1[0]; D.rec->scale = a2[0]; }
}

// chi2() > th || !isDepthPositive() (:680, :696, :723, :738): chi2 is the edge's LAST evaluation - a rejected trial's, and for an
// edge at level 1 round 1's -, the depth is computed at the current estimate.  final == 0: setLevel(1); final == 1: the erase flag.
__global__ __launch_bounds__(LBA_THREADS) void k_lba_classify(LbaDev D, int c, int final) {
    const int e = blockIdx.x * LBA_THREADS + threadIdx.x;
    if (e >= D.E) return;
    const orbb_observation_t o = D.obs[e];
    const double *T = D.pose[c] + (size_t)o.kf * 7, *Xp = D.pt[c] + (size_t)o.pt * 3;
    const double q[4] = {T[3], T[4], T[5], T[6]}, Xw[3] = {Xp[0], Xp[1], Xp[2]};
    double X[3];
    quat_rotate(q, Xw, X);
    const double z = X[2] + T[2];
    const bool out = D.chi2[e] > (o.ur < 0.f ? 5.991 : 7.815) || !(z > 0.0);
    if (final) D.erase[e] = out ? 1 : 0;
    else D.flag[e] = out ? 1 : 0;
}

// Converter::toCvMat(SE3Quat) and toCvMat(Vector3d) (:767, :777): a fixed keyframe, and everything when the call returns at :655,
// goes out as the bytes that came in; the double estimates beside them (q = x y z w, then t)
__global__ __launch_bounds__(LBA_THREADS) void k_lba_out(LbaDev D, int c, int untouched) {
    const int i = blockIdx.x * LBA_THREADS + threadIdx.x;
    if (i < D.K) {
        const double *T = D.pose[c] + (size_t)i * 7;
        float *to = D.outT + (size_t)i * 16;
        if (D.kf[i].fixed || untouched) {
            for (int k = 0; k < 16; k++) to[k] = D.kf[i].Tcw[k];
        } else {
            const double q[4] = {T[3], T[4], T[5], T[6]};
            double R[9];
            quat_to_R(q, R);
            for (int r = 0; r < 3; r++) {
                for (int cc = 0; cc < 3; cc++) to[r * 4 + cc] = (float)R[r * 3 + cc];
                to[r * 4 + 3] = (float)T[r];
            }
            to[12] = 0.f; to[13] = 0.f; to[14] = 0.f; to[15] = 1.f;
        }
        double *eo = D.estKf + (size_t)i * 7;
        eo[0] = T[3]; eo[1] = T[4]; eo[2] = T[5]; eo[3] = T[6]; eo[4] = T[0]; eo[5] = T[1]; eo[6] = T[2];
    }
    if (i < D.P) {
        const double *X = D.pt[c] + (size_t)i * 3;
        for (int k = 0; k < 3; k++) {
            D.outP[(size_t)i * 3 + k] = (float)X[k];   // the widened float narrows back to itself
            D.estPt[(size_t)i * 3 + k] = X[k];
        }
    }
}

// ------------------------------------------------------------------------------------
// the argument checks, before a device is touched
static inline bool lba_finite(float v) { return v >= -FLT_MAX && v <= FLT_MAX; }
static int lba_check(const char *fn, const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                     const orbb_schedule_t *s, float *Tcw_out, float *pts_out, uint8_t *erase) {
    if (K < 0 || P < 0 || E < 0 || !s || (K > 0 && (!kfs || !Tcw_out)) || (P > 0 && (!pts || !pts_out)) || (E > 0 && (!obs || !erase))) {
        orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG;
    }
    if ((s->rounds != 1 && s->rounds != 2) || !(s->delta_mono >= 0.f) || !lba_finite(s->delta_mono) || !(s->delta_stereo >= 0.f) || !lba_finite(s->delta_stereo)) {
        orbx_set_error("%s: bad schedule", fn); return ORBX_ERR_ARG;
    }
    for (int r = 0; r < s->rounds; r++)
        if (s->iterations[r] < 0 || s->iterations[r] > ORBB_MAX_ITERATIONS) { orbx_set_error("%s: iterations outside 0..%d", fn, ORBB_MAX_ITERATIONS); return ORBX_ERR_ARG; }
    for (int k = 0; k < K; k++) {
        bool ok = lba_finite(kfs[k].fx) && lba_finite(kfs[k].fy) && lba_finite(kfs[k].cx) && lba_finite(kfs[k].cy) && lba_finite(kfs[k].bf);
        for (int j = 0; j < 16; j++) ok = ok && lba_finite(kfs[k].Tcw[j]);
        if (!ok) { orbx_set_error("%s: keyframe %d is not finite", fn, k); return ORBX_ERR_ARG; }
    }
    for (int p = 0; p < P; p++)
        if (!lba_finite(pts[p].x) || !lba_finite(pts[p].y) || !lba_finite(pts[p].z)) { orbx_set_error("%s: point %d is not finite", fn, p); return ORBX_ERR_ARG; }
    std::vector<uint64_t> pairs((size_t)E);
    for (int e = 0; e < E; e++) {
        const orbb_observation_t &o = obs[e];
        if (o.kf < 0 || o.kf >= K || o.pt < 0 || o.pt >= P) { orbx_set_error("%s: observation %d names keyframe %d, point %d", fn, e, o.kf, o.pt); return ORBX_ERR_ARG; }
        if (!lba_finite(o.u) || !lba_finite(o.v) || !lba_finite(o.ur) || !(o.inv_sigma2 >= 0.f) || !lba_finite(o.inv_sigma2)) {
            orbx_set_error("%s: observation %d is not finite or its inv_sigma2 is negative", fn, e); return ORBX_ERR_ARG;
        }
        pairs[e] = ((uint64_t)(uint32_t)o.kf << 32) | (uint32_t)o.pt;
    }
    std::sort(pairs.begin(), pairs.end());
    for (int e = 1; e < E; e++)
        if (pairs[e] == pairs[e - 1]) {
            orbx_set_error("%s: keyframe %d observes point %d twice", fn, (int)(pairs[e] >> 32), (int)(uint32_t)pairs[e]); return ORBX_ERR_ARG;
        }
    return ORBX_OK;
}

// ------------------------------------------------------------------------------------
// The memory of one call and the four things the driver does with it.  The library: a device block, its pinned mirror and a stream
// (this thread's StagePair).  The lockstep program: one host block that is both, a launch is a loop over blockIdx.x.
struct LbaMem {
    uint8_t *d, *h;
#ifdef ORBX_LBA_HOST
    int push(size_t, size_t) { return ORBX_OK; }
    int fetch(size_t, size_t) { return ORBX_OK; }
    int fill(size_t off, int byte, size_t bytes) { memset(d + off, byte, bytes); return ORBX_OK; }
#else
    hipStream_t st;
    int push(size_t off, size_t bytes) { ORBX_HIP(hipMemcpyAsync(d + off, h + off, bytes, hipMemcpyHostToDevice, st)); return ORBX_OK; }
    int fetch(size_t off, size_t bytes) {   // the ONE synchronisation of a trial
        ORBX_HIP(hipMemcpyAsync(h + off, d + off, bytes, hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipStreamSynchronize(st));
        return ORBX_OK;
    }
    int fill(size_t off, int byte, size_t bytes) { ORBX_HIP(hipMemsetAsync(d + off, byte, bytes, st)); return ORBX_OK; }
#endif
};
#ifdef ORBX_LBA_HOST
#define LBA_LAUNCH(kern, grid, lds, ...) do { nlaunch++; for (int b_ = 0; b_ < (int)(grid); b_++) { blockIdx.x = b_; kern(__VA_ARGS__); } blockIdx.x = 0; } while (0)
#define LBA_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)
#else
#define LBA_LAUNCH(kern, grid, lds, ...) do { nlaunch++; hipLaunchKernelGGL(kern, dim3(grid), dim3(LBA_THREADS), lds, M.st, __VA_ARGS__); ORBX_HIP(hipGetLastError()); } while (0)
#define LBA_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)
#endif

struct LbaLayout {
    size_t oKf, oPts, oObs, oPtStart, oPtEdges, oKfStart, oKfEdges, inEnd, oCol, oKfOfCol, oFlag, oRec;
    size_t oOutT, oOutP, oErase, oEstKf, oEstPt, outEnd;
    size_t oPose[2], oPt[2], oPact, oChi2, oEd, oHll, oBl, oDinv, oDb, oHpp, oBp, oS, oXp, oPartChi, oPartScale, oTab, total;
    size_t oBlk, oBlkStart, oCa, oCb, oBad, nbMax, ncMax;   // the blocked path: the pattern and its contributions (uploaded per round), the pivot flag
    int nbE, nbK, nbP, nbAll, nfMax;
};
static inline int lba_blocks(int n) { return (n + LBA_THREADS - 1) / LBA_THREADS; }
// blocked (obs is read then): no [nf][P] table; room for the largest pattern a round can have, which is round 1's with every edge
// active - sum_p d_p (d_p + 1) / 2 contributions for d_p observations of point p by keyframes that are not fixed, and at most that
// many blocks and at most nf (nf + 1) / 2
static LbaLayout lba_layout(const orbb_keyframe_t *kfs, int K, int P, int E, const orbb_observation_t *obs = nullptr, int blocked = 0) {
    LbaLayout L;
    StagePlan pl;
    const size_t k1 = (size_t)(K > 0 ? K : 1), p1 = (size_t)(P > 0 ? P : 1), e1 = (size_t)(E > 0 ? E : 1);
    L.nfMax = 0;
    for (int k = 0; k < K; k++) L.nfMax += kfs[k].fixed ? 0 : 1;
    const size_t f1 = (size_t)(L.nfMax > 0 ? L.nfMax : 1);
    L.nbE = lba_blocks(E); L.nbK = lba_blocks(K); L.nbP = lba_blocks(P);
    L.nbAll = lba_blocks(std::max(K, std::max(P, E)));
    // uploaded once
    L.oKf = pl.take(k1 * sizeof(orbb_keyframe_t)); L.oPts = pl.take(p1 * sizeof(orbb_point_t)); L.oObs = pl.take(e1 * sizeof(orbb_observation_t));
    L.oPtStart = pl.take((p1 + 1) * 4); L.oPtEdges = pl.take(e1 * 4); L.oKfStart = pl.take((k1 + 1) * 4); L.oKfEdges = pl.take(e1 * 4);
    L.inEnd = pl.off;
    // uploaded per round; downloaded per round; downloaded per trial
    L.oCol = pl.take(k1 * 4); L.oKfOfCol = pl.take(k1 * 4); L.oFlag = pl.take(e1); L.oRec = pl.take(sizeof(LbaRec));
    // downloaded at the end
    L.oOutT = pl.take(k1 * 64); L.oOutP = pl.take(p1 * 12); L.oErase = pl.take(e1); L.oEstKf = pl.take(k1 * 56); L.oEstPt = pl.take(p1 * 24);
    L.outEnd = pl.off;
    // device only
    for (int i = 0; i < 2; i++) { L.oPose[i] = pl.take(k1 * 56); L.oPt[i] = pl.take(p1 * 24); }
    L.oPact = pl.take(p1); L.oChi2 = pl.take(e1 * 8); L.oEd = pl.take(e1 * LBA_ED * 8);
    L.oHll = pl.take(p1 * 48); L.oBl = pl.take(p1 * 24); L.oDinv = pl.take(p1 * 48); L.oDb = pl.take(p1 * 24);
    L.oHpp = pl.take(f1 * 168); L.oBp = pl.take(f1 * 48); L.oS = pl.take(f1 * f1 * 36 * 8); L.oXp = pl.take(f1 * 48);
    L.oPartChi = pl.take((size_t)(L.nbE > 0 ? L.nbE : 1) * 8); L.oPartScale = pl.take((size_t)(L.nbK + L.nbP > 0 ? L.nbK + L.nbP : 1) * 8);
    L.oTab = pl.take(blocked ? 0 : f1 * p1 * 4);
    L.nbMax = L.ncMax = 0;
    if (blocked) {
        std::vector<size_t> deg((size_t)P, 0);
        for (int e = 0; e < E; e++)
            if (!kfs[obs[e].kf].fixed) deg[obs[e].pt]++;
        for (int p = 0; p < P; p++) L.ncMax += deg[p] * (deg[p] + 1) / 2;
        L.nbMax = std::min(L.ncMax, (size_t)L.nfMax * ((size_t)L.nfMax + 1) / 2);
    }
    L.oBlk = pl.take((L.nbMax + 1) * 8); L.oBlkStart = pl.take((L.nbMax + 1) * 8);
    L.oCa = pl.take((L.ncMax + 1) * 4); L.oCb = pl.take((L.ncMax + 1) * 4); L.oBad = pl.take(4);
    L.total = pl.off;
    return L;
}

// The blocked path's pattern of a round, into the mirror: the blocks (i1 <= i2) that share an active point, sorted, and per block
// its contributions (edge of i1, edge of i2) in ascending point index - the order of tests/lba_ref.py: Round.sum_schur.  Column by
// column: the column's active edges sorted by point, each paired with the point's active edges in columns >= i1 (a diagonal block
// pairs an edge with itself).  Two passes over the same walk, count and place.  -> the number of blocks, contributions in *nc.
static size_t gba_pattern(uint8_t *h, const LbaLayout &L, int nf, bool useFlag, size_t *nc) {
    const orbb_observation_t *obs = (const orbb_observation_t *)(h + L.oObs);
    const int32_t *ptStart = (const int32_t *)(h + L.oPtStart), *ptEdges = (const int32_t *)(h + L.oPtEdges);
    const int32_t *kfStart = (const int32_t *)(h + L.oKfStart), *kfEdges = (const int32_t *)(h + L.oKfEdges);
    const int32_t *col = (const int32_t *)(h + L.oCol), *kfOfCol = (const int32_t *)(h + L.oKfOfCol);
    const uint8_t *flag = h + L.oFlag;
    int32_t *blk = (int32_t *)(h + L.oBlk), *ca = (int32_t *)(h + L.oCa), *cb = (int32_t *)(h + L.oCb);
    long long *blkStart = (long long *)(h + L.oBlkStart);
    std::vector<long long> cnt((size_t)nf, 0);
    std::vector<int32_t> touched;
    std::vector<std::pair<int32_t, int32_t> > mine;   // (point, edge) of the column
    size_t nb = 0;
    long long run = 0;
    for (int i1 = 0; i1 < nf; i1++) {
        const int kf = kfOfCol[i1];
        mine.clear(); touched.clear();
        for (int i = kfStart[kf]; i < kfStart[kf + 1]; i++) {
            const int e = kfEdges[i];
            if (!(useFlag && flag[e])) mine.push_back(std::make_pair(obs[e].pt, e));
        }
        std::sort(mine.begin(), mine.end());
        for (int pass = 0; pass < 2; pass++) {
            for (size_t a = 0; a < mine.size(); a++) {
                const int p = mine[a].first;
                for (int i = ptStart[p]; i < ptStart[p + 1]; i++) {
                    const int eb = ptEdges[i];
                    if (useFlag && flag[eb]) continue;
                    const int i2 = col[obs[eb].kf];
                    if (i2 < i1) continue;   // a fixed keyframe (-1), or the block belongs to column i2
                    if (pass == 0) { if (cnt[i2]++ == 0) touched.push_back(i2); }
                    else { ca[cnt[i2]] = mine[a].second; cb[cnt[i2]] = eb; cnt[i2]++; }
                }
            }
            if (pass == 0) {
                std::sort(touched.begin(), touched.end());
                for (size_t k = 0; k < touched.size(); k++) {
                    const int i2 = touched[k];
                    blk[2 * nb] = i1; blk[2 * nb + 1] = i2; blkStart[nb] = run;
                    const long long c = cnt[i2];
                    cnt[i2] = run;            // pass 1 places from here
                    run += c; nb++;
                }
            } else {
                for (size_t k = 0; k < touched.size(); k++) cnt[touched[k]] = 0;
            }
        }
    }
    blkStart[nb] = run;
    *nc = (size_t)run;
    return nb;
}

typedef int (*lba_stop_fn)(void *);
// The schedule of :655-707 and the Levenberg-Marquardt of optimization_algorithm_levenberg.cpp:61-164 under sparse_optimizer.cpp:376.
// M.h holds the inputs on entry (lba_stage) and the outputs on return.  The loops are bounded by the schedule: iterations x 10 trials.
static int lba_drive(LbaMem M, const LbaLayout &L, int K, int P, int E, const orbb_schedule_t &sc, lba_stop_fn stop, void *user, orbb_info_t *info,
                     int blocked = 0, orbb_blocked_info_t *binfo = nullptr) {
    LbaDev D;
    uint8_t *d = M.d;
    D.K = K; D.P = P; D.E = E; D.nf = 0;
    D.kf = (const orbb_keyframe_t *)(d + L.oKf); D.pts = (const orbb_point_t *)(d + L.oPts); D.obs = (const orbb_observation_t *)(d + L.oObs);
    D.ptStart = (const int32_t *)(d + L.oPtStart); D.ptEdges = (const int32_t *)(d + L.oPtEdges);
    D.kfStart = (const int32_t *)(d + L.oKfStart); D.kfEdges = (const int32_t *)(d + L.oKfEdges);
    D.col = (const int32_t *)(d + L.oCol); D.kfOfCol = (const int32_t *)(d + L.oKfOfCol); D.tab = (int32_t *)(d + L.oTab);
    for (int i = 0; i < 2; i++) { D.pose[i] = (double *)(d + L.oPose[i]); D.pt[i] = (double *)(d + L.oPt[i]); }
    D.flag = d + L.oFlag; D.erase = d + L.oErase; D.pact = d + L.oPact;
    D.chi2 = (double *)(d + L.oChi2); D.ed = (double *)(d + L.oEd); D.Hll = (double *)(d + L.oHll); D.bl = (double *)(d + L.oBl);
    D.Dinv = (double *)(d + L.oDinv); D.db = (double *)(d + L.oDb); D.Hpp = (double *)(d + L.oHpp); D.bp = (double *)(d + L.oBp);
    D.S = (double *)(d + L.oS); D.xp = (double *)(d + L.oXp); D.partChi = (double *)(d + L.oPartChi); D.partScale = (double *)(d + L.oPartScale);
    D.rec = (LbaRec *)(d + L.oRec);
    D.outT = (float *)(d + L.oOutT); D.outP = (float *)(d + L.oOutP); D.estKf = (double *)(d + L.oEstKf); D.estPt = (double *)(d + L.oEstPt);
    const orbb_keyframe_t *hkf = (const orbb_keyframe_t *)(M.h + L.oKf);
    const orbb_observation_t *hobs = (const orbb_observation_t *)(M.h + L.oObs);
    int32_t *hcol = (int32_t *)(M.h + L.oCol), *hkfOfCol = (int32_t *)(M.h + L.oKfOfCol);
    const uint8_t *hflag = M.h + L.oFlag;
    const LbaRec *hrec = (const LbaRec *)(M.h + L.oRec);

    D.blk = (const int32_t *)(d + L.oBlk); D.blkStart = (const long long *)(d + L.oBlkStart);
    D.ca = (const int32_t *)(d + L.oCa); D.cb = (const int32_t *)(d + L.oCb); D.bad = (int32_t *)(d + L.oBad);
    orbb_info_t inf;
    memset(&inf, 0, sizeof(inf));
    orbb_blocked_info_t bi;
    memset(&bi, 0, sizeof(bi));
    long long nlaunch = 0;   // LBA_LAUNCH counts
    int polls = 0;
    auto poll = [&](int where) -> bool {   // OptimizableGraph::terminate(), and the reference's own two reads of the flag
        if (!stop) return false;
        polls++;
        const bool s = stop(user) != 0;
        if (s && !inf.stopped_at) { inf.stopped_at = where; inf.stop_poll = polls; }
        return s;
    };
    LBA_TRY(M.push(0, L.inEnd));
    if (L.nbAll) LBA_LAUNCH(k_lba_init, L.nbAll, 0, D);
    int c = 0;
    bool untouched = false, classify = sc.classify != 0;
    if (sc.check_stop_first && poll(ORBB_STOP_BEFORE)) { untouched = true; classify = false; }   // :655: return, nothing written
    for (int round = 0; round < sc.rounds && !untouched; round++) {
        if (round == 1) {
            if (poll(ORBB_STOP_BETWEEN)) break;   // :664: bDoMore = false
            if (L.nbE) LBA_LAUNCH(k_lba_classify, L.nbE, 0, D, c, 0);
            LBA_TRY(M.fetch(L.oFlag, (size_t)(E > 0 ? E : 1)));
        }
        // initializeOptimization(0): a vertex without an edge at level 0 is not in the problem (sparse_optimizer.cpp:218-259)
        int nActive = 0, nf = 0;
        for (int k = 0; k < K; k++) hcol[k] = hkf[k].fixed ? -1 : -2;
        for (int e = 0; e < E; e++) {
            if (round == 1 && hflag[e]) continue;
            nActive++;
            if (hcol[hobs[e].kf] == -2) hcol[hobs[e].kf] = -3;
        }
        for (int k = 0; k < K; k++) {
            if (hcol[k] == -3) { hkfOfCol[nf] = k; hcol[k] = nf++; }
            else hcol[k] = -1;
        }
        inf.rounds = round + 1;
        inf.free_poses[round] = nf;
        if (!nActive) continue;   // optimize(): "0 vertices to optimize", no iteration and no poll
        D.nf = nf;
        LBA_TRY(M.push(L.oCol, L.oFlag - L.oCol));
        const int n = nf * 6, panels = (nf + GBA_PANEL_POSES - 1) / GBA_PANEL_POSES;
        size_t nb = 0, nc = 0;
        if (blocked) {
            nb = gba_pattern(M.h, L, nf, round == 1, &nc);
            bi.blocks[round] = (int32_t)nb; bi.panels[round] = panels; bi.contributions[round] = (int64_t)nc;
            LBA_TRY(M.push(L.oBlk, (nb + 1) * 8)); LBA_TRY(M.push(L.oBlkStart, (nb + 1) * 8));
            LBA_TRY(M.push(L.oCa, (nc + 1) * 4)); LBA_TRY(M.push(L.oCb, (nc + 1) * 4));
        } else if (nf) {
            LBA_TRY(M.fill(L.oTab, 0xFF, (size_t)nf * P * 4));
            LBA_LAUNCH(k_lba_table, L.nbE, 0, D);
        }
        const int inLds = nf <= LBA_LDS_POSES;
        const size_t lds = inLds ? (size_t)nf * nf * 36 * 8 : 0;
        (void)lds;
        const int robust = sc.robust[round] != 0;
        const double dMono = (double)sc.delta_mono, dStereo = (double)sc.delta_stereo;
        const int where = round == 0 ? ORBB_STOP_ROUND1 : ORBB_STOP_ROUND2;
        double lambda = 0.0, ni = 2.0;
        int nbadIt = 0;
        bool ok = true;
        for (int it = 0; it < sc.iterations[round]; it++) {
            if (poll(where) || !ok) break;   // for (i = 0; i < iterations && !terminate() && ok; i++)
            LBA_LAUNCH(k_lba_edges<true>, L.nbE, 0, D, c, robust, dMono, dStereo);
            LBA_LAUNCH(k_lba_point, L.nbP, 0, D);
            if (nf) LBA_LAUNCH(k_lba_pose, nf, 0, D);
            LBA_LAUNCH(k_lba_lin_reduce, 1, 0, D, L.nbE);
            if (it == 0) {   // computeLambdaInit: tau * max |diagonal|
                LBA_TRY(M.fetch(L.oRec, sizeof(LbaRec)));
                lambda = 1e-5 * hrec->maxDiag; ni = 2.0; nbadIt = 0;
            }
            double cur = 0.0, iniChi = 0.0, rho = 0.0;
            int q = 0;
            bool more;
            do {
                LBA_LAUNCH(k_lba_dinv, L.nbP, 0, D, lambda);
                if (blocked) {
                    // S and the pivot flag start every trial as zeros: a block outside the pattern is zero, not scratch
                    LBA_TRY(M.fill(L.oS, 0, (size_t)n * (size_t)n * 8)); LBA_TRY(M.fill(L.oBad, 0, 4));
                    if (nb) LBA_LAUNCH(k_gba_schur, nb, 0, D, lambda);
                    for (int c0 = 0; c0 < n; c0 += GBA_NB) {
                        const int w = std::min(GBA_NB, n - c0), below = n - c0 - w, tiles = (below + GBA_TILE - 1) / GBA_TILE;
                        LBA_LAUNCH(k_gba_diag, 1, 0, D, n, c0, w);
                        if (below > 0) {
                            LBA_LAUNCH(k_gba_rows, lba_blocks(below), 0, D, n, c0);
                            LBA_LAUNCH(k_gba_trail, tiles * (tiles + 1) / 2, 0, D, n, c0);
                        }
                    }
                    if (n) LBA_LAUNCH(k_gba_scale, lba_blocks(n), 0, D, n);
                    for (int c0 = (panels - 1) * GBA_NB; c0 >= 0 && n; c0 -= GBA_NB) {
                        const int w = std::min(GBA_NB, n - c0);
                        LBA_LAUNCH(k_gba_back_diag, 1, 0, D, n, c0, w);
                        if (c0 > 0) LBA_LAUNCH(k_gba_back_rows, lba_blocks(c0), 0, D, n, c0, w);
                    }
                    LBA_LAUNCH(k_gba_finish, std::max(1, lba_blocks(n)), 0, D, n);
                } else {
                    if (nf) LBA_LAUNCH(k_lba_schur, nf * nf, 0, D, lambda);
                    LBA_LAUNCH(k_lba_solve, 1, lds, D, inLds);
                }
                LBA_LAUNCH(k_lba_update, L.nbK + L.nbP, 0, D, c, lambda, L.nbK);
                LBA_LAUNCH(k_lba_edges<false>, L.nbE, 0, D, c ^ 1, robust, dMono, dStereo);
                LBA_LAUNCH(k_lba_trial_reduce, 1, 0, D, L.nbE, L.nbK + L.nbP);
                LBA_TRY(M.fetch(L.oRec, sizeof(LbaRec)));
                if (q == 0) { cur = hrec->linChi; iniChi = cur; }
                double tmp = hrec->tmpChi;
                if (!hrec->ok) tmp = DBL_MAX;
                const double scale = hrec->scale + 1e-3;
                rho = (cur - tmp) / scale;
                if (rho > 0.0 && fabs(tmp) <= DBL_MAX) {
                    const double u = 2.0 * rho - 1.0;
                    double alpha = 1.0 - (u * u) * u;
                    alpha = fmin(alpha, 2.0 / 3.0);
                    lambda *= fmax(1.0 / 3.0, alpha);
                    ni = 2.0;
                    cur = tmp;
                    c ^= 1;   // discardTop: the trial estimates are the current ones
                } else {
                    lambda *= ni;
                    ni *= 2.0;   // pop: the current estimates stand
                }
                q++;
                more = rho < 0.0 && q < LBA_MAX_TRIALS;
                if (more && poll(where)) more = false;
            } while (more);
            inf.iterations[round]++; inf.trials[round] += q;
            if (q == LBA_MAX_TRIALS || rho == 0.0) { ok = false; continue; }   // Terminate: the loop's condition is read once more
            if ((iniChi - cur) * 1e3 < iniChi) nbadIt++; else nbadIt = 0;      // the reference's own stop criterion
            if (nbadIt >= 3) ok = false;
        }
    }
    if (classify && L.nbE) LBA_LAUNCH(k_lba_classify, L.nbE, 0, D, c, 1);
    if (L.nbAll) LBA_LAUNCH(k_lba_out, L.nbAll, 0, D, c, untouched ? 1 : 0);
    LBA_TRY(M.fetch(L.oOutT, L.outEnd - L.oOutT));
    inf.polls = polls;
    const uint8_t *er = M.h + L.oErase;
    for (int e = 0; e < E; e++) inf.erased += er[e];
    if (info) *info = inf;
    bi.launches = nlaunch;
    if (binfo) *binfo = bi;
    return ORBX_OK;
}

// the inputs into the mirror, and the per-owner lists: CSR by point and by keyframe, an owner's edges in ascending input index
static void lba_stage(uint8_t *h, const LbaLayout &L, const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E) {
    if (K) memcpy(h + L.oKf, kfs, (size_t)K * sizeof(orbb_keyframe_t));
    if (P) memcpy(h + L.oPts, pts, (size_t)P * sizeof(orbb_point_t));
    if (E) memcpy(h + L.oObs, obs, (size_t)E * sizeof(orbb_observation_t));
    int32_t *ps = (int32_t *)(h + L.oPtStart), *pe = (int32_t *)(h + L.oPtEdges), *ks = (int32_t *)(h + L.oKfStart), *ke = (int32_t *)(h + L.oKfEdges);
    for (int p = 0; p <= P; p++) ps[p] = 0;
    for (int k = 0; k <= K; k++) ks[k] = 0;
    for (int e = 0; e < E; e++) { ps[obs[e].pt + 1]++; ks[obs[e].kf + 1]++; }
    for (int p = 0; p < P; p++) ps[p + 1] += ps[p];
    for (int k = 0; k < K; k++) ks[k + 1] += ks[k];
    std::vector<int32_t> pn(ps, ps + P), kn(ks, ks + K);
    for (int e = 0; e < E; e++) { pe[pn[obs[e].pt]++] = e; ke[kn[obs[e].kf]++] = e; }
    memset(h + L.oErase, 0, (size_t)(E > 0 ? E : 1));
}
static void lba_results(const uint8_t *h, const LbaLayout &L, int K, int P, int E, float *Tcw_out, float *pts_out, uint8_t *erase, double *kf_est, double *pt_est) {
    if (K) memcpy(Tcw_out, h + L.oOutT, (size_t)K * 64);
    if (P) memcpy(pts_out, h + L.oOutP, (size_t)P * 12);
    if (E) memcpy(erase, h + L.oErase, (size_t)E);
    if (kf_est && K) memcpy(kf_est, h + L.oEstKf, (size_t)K * 56);
    if (pt_est && P) memcpy(pt_est, h + L.oEstPt, (size_t)P * 24);
}

#ifndef ORBX_LBA_HOST
// host side: this thread's staging pair (orbx_stage.h)
static thread_local StagePair g_ba;
void orbx_internal_release_lba_scratch() { g_ba.release(); }

// one call on this thread's staging pair; blocked: the k_gba_* reduced-system path
static int lba_run(const char *fn, const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                   const orbb_schedule_t *schedule, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                   uint8_t *erase, orbb_info_t *info, double *kf_est7, double *pt_est3, int blocked, orbb_blocked_info_t *binfo, int device) {
    const int crc = lba_check(fn, kfs, K, pts, P, obs, E, schedule, Tcw_out16, pts_out3, erase);
    if (crc) return crc;
    const LbaLayout L = lba_layout(kfs, K, P, E, obs, blocked);
    int rc = g_ba.reserve(device, L.total, (size_t)1 << 20);
    if (rc) return rc;
    LbaMem M;
    M.d = g_ba.d; M.h = g_ba.h; M.st = g_ba.stream;
    lba_stage(M.h, L, kfs, K, pts, P, obs, E);
    (void)hipGetLastError();
    rc = lba_drive(M, L, K, P, E, *schedule, stop, stop_user, info, blocked, binfo);
    if (rc) { hipStreamSynchronize(M.st); return rc; }
    lba_results(M.h, L, K, P, E, Tcw_out16, pts_out3, erase, kf_est7, pt_est3);
    return ORBX_OK;
}

extern "C" int orbb_optimize(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                             const orbb_schedule_t *schedule, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                             uint8_t *erase, orbb_info_t *info, double *kf_est7, double *pt_est3, int device) {
    return lba_run("orbb_optimize", kfs, K, pts, P, obs, E, schedule, stop, stop_user, Tcw_out16, pts_out3, erase, info, kf_est7, pt_est3, 0, nullptr, device);
}

extern "C" int orbb_optimize_blocked(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                                     const orbb_schedule_t *schedule, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                                     uint8_t *erase, orbb_info_t *info, double *kf_est7, double *pt_est3, orbb_blocked_info_t *binfo, int device) {
    return lba_run("orbb_optimize_blocked", kfs, K, pts, P, obs, E, schedule, stop, stop_user, Tcw_out16, pts_out3, erase, info, kf_est7, pt_est3, 1, binfo, device);
}

extern "C" int orbb_local_bundle_adjustment(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                                            int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3, uint8_t *erase,
                                            orbb_info_t *info, double *kf_est7, double *pt_est3, int device) {
    // optimize(5) with the Huber kernel, the classification, optimize(10) without it over the edges left at level 0 (:569-570, :660-707)
    const orbb_schedule_t s = {2, {5, 10}, {1, 0}, (float)sqrt(5.991), (float)sqrt(7.815), 1, 1};
    return orbb_optimize(kfs, K, pts, P, obs, E, &s, stop, stop_user, Tcw_out16, pts_out3, erase, info, kf_est7, pt_est3, device);
}

extern "C" int orbb_bundle_adjustment(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                                      int iterations, int robust, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                                      orbb_info_t *info, double *kf_est7, double *pt_est3, int device) {
    // one optimize(nIterations), no classification; thHuber2D = sqrt(5.99) here, not 5.991 (:95-96)
    const orbb_schedule_t s = {1, {iterations, 0}, {robust ? 1 : 0, 0}, (float)sqrt(5.99), (float)sqrt(7.815), 0, 0};
    std::vector<uint8_t> erase((size_t)(E > 0 ? E : 1));
    return orbb_optimize(kfs, K, pts, P, obs, E, &s, stop, stop_user, Tcw_out16, pts_out3, erase.data(), info, kf_est7, pt_est3, device);
}

extern "C" int orbb_global_bundle_adjustment(const orbb_keyframe_t *kfs, int K, const orbb_point_t *pts, int P, const orbb_observation_t *obs, int E,
                                             int iterations, int robust, int (*stop)(void *), void *stop_user, float *Tcw_out16, float *pts_out3,
                                             orbb_info_t *info, double *kf_est7, double *pt_est3, orbb_blocked_info_t *binfo, int device) {
    // orbb_bundle_adjustment's schedule (:95-96) on the blocked path
    const orbb_schedule_t s = {1, {iterations, 0}, {robust ? 1 : 0, 0}, (float)sqrt(5.99), (float)sqrt(7.815), 0, 0};
    std::vector<uint8_t> erase((size_t)(E > 0 ? E : 1));
    return orbb_optimize_blocked(kfs, K, pts, P, obs, E, &s, stop, stop_user, Tcw_out16, pts_out3, erase.data(), info, kf_est7, pt_est3, binfo, device);
}
#endif   // ORBX_LBA_HOST
