// orbx_essential.hip — Optimizer::OptimizeEssentialGraph (reference: src/Optimizer.cc:783-1049): one VertexSim3Expmap per keyframe,
// one EdgeSim3 per edge of the essential graph (identity information, no robust kernel, g2o's NUMERIC Jacobians with delta = 1e-9),
// Levenberg-Marquardt from lambda = 1e-16 over the whole Hpp.  A restatement of the reference and of the g2o classes it drives
// (types/sim3.h, types_seven_dof_expmap.h, base_binary_edge.hpp, block_solver.hpp, optimization_algorithm_levenberg), double
// throughout; DESIGN.md section 6, "k_eg_*", has the list.  tests/essential_ref.py is the same arithmetic in numpy.
//
// The block pattern is the same in every iteration, so the HOST does the symbolic half once per call (eg_symbolic): natural order
// of the free vertices, elimination tree, the pattern of the factor with fill, for every factor block the list of updates it
// receives, the levels of the tree.  The device does the numeric half: a block LDL^T without pivoting, left-looking, ONE workgroup
// per column, the columns of one level of the elimination tree in one launch; the two substitutions level by level likewise.  The
// host drives iterations and trials (eg_drive) and reads one small record per trial - one stream synchronisation, none device-wide.
// No cooperative launch, no wait loop in a kernel, no floating-point atomics.  Every sum has one owner and a fixed order:
//   a Jacobian column           one thread: both signs of the step                                              (k_eg_edges<true>)
//   Hii / b, one row            one thread: the vertex's edges in ascending input index                         (k_eg_vertex)
//   Hij, one row                one thread: the pair's edges in ascending input index                           (k_eg_offdiag)
//   a factor entry              one thread of the column's workgroup: its updates in ascending column order     (k_eg_factor)
//   y / x of a column           one thread: the row's / column's blocks in ascending order                      (k_eg_forward, k_eg_backward)
//   chi2, computeScale          per-workgroup partial sums, then one workgroup over the partials in order        (k_eg_reduce)
// so two runs give the same bytes.
#ifdef ORBX_EG_HOST
// tests/cpp/essential_lockstep.cc compiles this file's kernels AND the driver for the host, one thread per workgroup, the
// workgroups of a launch one after the other (tests/cpp/hip_lockstep.h comes first): every sum then runs in ascending order, which
// is tests/essential_ref.py's order - the two must agree bit for bit (tests/test_essential_cpu.py).
#include "orbx_stage_plan.h"
#define EG_THREADS 1
#define EG_LANES 1
#else
#include "orbx_stage.h"
#define EG_THREADS 256
#define EG_LANES 64
#endif
#include <float.h>
#include <math.h>
#include <algorithm>
#include <vector>
#include "orbx_g2omath.h"

#define EG_WAVES ((EG_THREADS + EG_LANES - 1) / EG_LANES)
#define EG_SLOTS 16         // threads an edge gets in a linearisation: 7 columns of side i | 7 of side j | the error itself | idle
#define EG_MAX_TRIALS 10    // g2o's maxTrialsAfterFailure
#define EG_DELTA 1e-9       // base_binary_edge.hpp:147

typedef orbg_sim3_t EgS3;
struct EgRec { double linChi, tmpChi, scale; int32_t ok, pad; };   // what the host reads after every trial
struct EgDev {
    int32_t N, E, P, nf, nblk, noff, fixScale, pad;
    const orbg_vertex_t *vtx; const orbg_edge_t *edges; const orbg_point_t *pts;
    const int32_t *colOf, *vtxOfCol;          // vertex -> column (-1: fixed, or no edge) and back
    const int32_t *vStart, *vEdges;           // CSR by column: the edges at its vertex in ascending input index
    const int32_t *oRow, *oCol, *oStart, *oEdges;   // the pairs of free vertices with an edge (row column > column column), their edges ascending
    const int32_t *colStart, *blkRow, *blkCol, *blkSrc;   // the factor: a column's blocks (the diagonal one first, then ascending row); blkSrc: pair or -1 (fill)
    const int32_t *updStart, *updA, *updB, *updD;         // per block (r, c): for ascending k the blocks (r, k), (c, k) and k's diagonal block
    const int32_t *rowStart, *rowBlk;         // per column c: the blocks (c, k), k < c ascending
    const int32_t *lvlCols;                   // the columns level by level, ascending inside a level
    EgS3 *est[2], *meas;                      // the estimates, current and trial, swapped by the host; the measurement of every edge
    double *err, *jac, *Hd, *b, *Hoff, *L, *x, *partChi, *partScale;
    EgRec *rec;
    float *outT, *outP; double *outE;
};
// block_sum and the quaternion and Sim3 functions (sim3_mul, sim3_inverse, sim3_map, sim3_exp) are orbx_g2omath.h's

// W.lu().solve(t) for a 3x3 W: partial pivoting - in column k the row of the largest |entry| among rows k.., the FIRST one on a
// tie - then the unit lower and the upper substitution.  A zero pivot divides by zero as Eigen's does.
__device__ __forceinline__ void eg_lu3_solve(double W[9], const double t[3], double x[3]) {
    double b[3] = {t[0], t[1], t[2]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int p = k;
        double best = fabs(W[k * 3 + k]);
#pragma unroll
        for (int r = k + 1; r < 3; r++) {
            const double a = fabs(W[r * 3 + k]);
            if (a > best) { best = a; p = r; }
        }
#pragma unroll
        for (int r = k + 1; r < 3; r++)   // the swap of rows k and p, every index a constant once unrolled
            if (p == r) {
#pragma unroll
                for (int c = 0; c < 3; c++) { const double s = W[k * 3 + c]; W[k * 3 + c] = W[r * 3 + c]; W[r * 3 + c] = s; }
                const double s = b[k]; b[k] = b[r]; b[r] = s;
            }
        const double piv = W[k * 3 + k];
#pragma unroll
        for (int r = k + 1; r < 3; r++) {
            W[r * 3 + k] = W[r * 3 + k] / piv;
#pragma unroll
            for (int c = k + 1; c < 3; c++) W[r * 3 + c] -= W[r * 3 + k] * W[k * 3 + c];
        }
    }
    b[1] -= W[3] * b[0];
    b[2] -= W[6] * b[0];
    b[2] -= W[7] * b[1];
    x[2] = b[2] / W[8];
    x[1] = (b[1] - W[5] * x[2]) / W[4];
    x[0] = ((b[0] - W[1] * x[1]) - W[2] * x[2]) / W[0];
}
// Sim3::log (sim3.h:148-230) -> omega | upsilon | sigma, its four branches as written.  B of the branch |sigma| >= eps, d > 1 - eps
// is line 199's, ((0.5 sigma^2 - sigma + 1) s) / sigma^3: of order 1 / sigma^3 (DESIGN.md says what follows from that).
__device__ __forceinline__ void eg_log(const EgS3 &S, double res[7]) {
    const double sigma = log(S.s);
    double R[9];
    quat_to_R(S.q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const double eps = 0.00001;
    double A, B, Cc, k;
    if (fabs(sigma) < eps) {
        Cc = 1.0;
        if (d > 1.0 - eps) {
            k = 0.5; A = 1. / 2.; B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta;
            k = theta / (2.0 * sqrt(1.0 - d * d));
            A = (1.0 - cos(theta)) / theta2;
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        Cc = (S.s - 1.0) / sigma;
        if (d > 1.0 - eps) {
            const double sigma2 = sigma * sigma;
            k = 0.5;
            A = ((sigma - 1.0) * S.s + 1.0) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1.0) * S.s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            k = theta / (2.0 * sqrt(1.0 - d * d));
            const double theta2 = theta * theta, a = S.s * sin(theta), b = S.s * cos(theta), c = theta2 + sigma * sigma;
            A = (a * sigma + (1.0 - b) * theta) / (theta * c);
            B = ((Cc - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2;
        }
    }
    const double o0 = k * dR[0], o1 = k * dR[1], o2 = k * dR[2];
    const double Om[9] = {0.0, -o2, o1, o2, 0.0, -o0, -o1, o0, 0.0};
    double W[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double om2 = (Om[r * 3] * Om[c] + Om[r * 3 + 1] * Om[3 + c]) + Om[r * 3 + 2] * Om[6 + c];
            W[r * 3 + c] = (A * Om[r * 3 + c] + B * om2) + Cc * (r == c ? 1.0 : 0.0);
        }
    double ups[3];
    eg_lu3_solve(W, S.t, ups);
    res[0] = o0; res[1] = o1; res[2] = o2; res[3] = ups[0]; res[4] = ups[1]; res[5] = ups[2]; res[6] = sigma;
}
// EdgeSim3::computeError (types_seven_dof_expmap.h:106-114): (C * v1 * v2^-1).log()
__device__ __forceinline__ void eg_error(const EgS3 &Cm, const EgS3 &Si, const EgS3 &Sj, double e[7]) {
    eg_log(sim3_mul(sim3_mul(Cm, Si), sim3_inverse(Sj)), e);
}

// the estimates as the reference sets them (:820-834) and every edge's measurement (:859-869, :891-916)
__global__ __launch_bounds__(EG_THREADS) void k_eg_init(EgDev D) {
    const int i = blockIdx.x * EG_THREADS + threadIdx.x;
    if (i < D.N) { D.est[0][i] = D.vtx[i].Scw; D.est[1][i] = D.vtx[i].Scw; }
    if (i < D.E) {
        const orbg_edge_t e = D.edges[i];
        const orbg_vertex_t *vi = D.vtx + e.i, *vj = D.vtx + e.j;
        const bool nc = e.kind != 0;
        const EgS3 Siw = (nc && vi->has_nc) ? vi->Snc : vi->Scw, Sjw = (nc && vj->has_nc) ? vj->Snc : vj->Scw;
        D.meas[i] = sim3_mul(Sjw, sim3_inverse(Siw));
    }
}

// LIN: EG_SLOTS threads per edge at estimate `c`.  Slots 0..13: column (slot % 7) of the Jacobian of side (slot / 7), the central
// difference of linearizeOplus (base_binary_edge.hpp:131-205) through oplusImpl (update[6] = 0 under fix_scale, so that column is
// e - e = 0 exactly); the side of a fixed vertex is skipped.  Slot 14: computeError and chi2 = e . e, into the workgroup's partial
// sum.  !LIN: one thread per edge, the error and chi2 alone.
template <bool LIN>
__global__ __launch_bounds__(EG_THREADS) void k_eg_edges(EgDev D, int c) {
    __shared__ double part[EG_WAVES];
    const int item = blockIdx.x * EG_THREADS + threadIdx.x;
    const int e = LIN ? item / EG_SLOTS : item, slot = LIN ? item % EG_SLOTS : 14;
    double chi = 0.0;
    if (e < D.E && slot < 15) {
        const orbg_edge_t ed = D.edges[e];
        const EgS3 Cm = D.meas[e], Si = D.est[c][ed.i], Sj = D.est[c][ed.j];
        if (slot == 14) {
            double er[7];
            eg_error(Cm, Si, Sj, er);
#pragma unroll
            for (int k = 0; k < 7; k++) { D.err[(size_t)e * 7 + k] = er[k]; chi += er[k] * er[k]; }
        } else {
            const int side = slot / 7, col = slot % 7;
            if (!D.vtx[side ? ed.j : ed.i].fixed) {
                double e2[2][7], u[7];
#pragma unroll
                for (int s = 0; s < 2; s++) {
#pragma unroll
                    for (int k = 0; k < 7; k++) u[k] = k == col ? (s ? -EG_DELTA : EG_DELTA) : 0.0;
                    if (D.fixScale) u[6] = 0.0;
                    const EgS3 Sp = sim3_mul(sim3_exp(u), side ? Sj : Si);
                    const EgS3 Sa = side ? Si : Sp, Sb = side ? Sp : Sj;
                    eg_error(Cm, Sa, Sb, e2[s]);
                }
                const double scalar = 1.0 / (2 * EG_DELTA);
                double *J = D.jac + ((size_t)e * 2 + side) * 49;
#pragma unroll
                for (int k = 0; k < 7; k++) J[k * 7 + col] = scalar * (e2[0][k] - e2[1][k]);
            }
        }
    }
    chi = block_sum<EG_LANES, EG_WAVES>(chi, part);
    if (threadIdx.x == 0) D.partChi[blockIdx.x] = chi;
}

// constructQuadraticForm (base_binary_edge.hpp:55-120) with identity information, the diagonal part: row r of Hii and b[r] of the
// vertex of column item / 7, over the vertex's edges in ascending input index; A^T A and A^T (-e), the inner sums over the residual
__global__ __launch_bounds__(EG_THREADS) void k_eg_vertex(EgDev D) {
    const int item = blockIdx.x * EG_THREADS + threadIdx.x;
    const int col = item / 7, r = item % 7;
    if (col >= D.nf) return;
    const int v = D.vtxOfCol[col];
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = D.vStart[col]; i < D.vStart[col + 1]; i++) {
        const int e = D.vEdges[i];
        const double *J = D.jac + ((size_t)e * 2 + (D.edges[e].i == v ? 0 : 1)) * 49, *er = D.err + (size_t)e * 7;
#pragma unroll
        for (int cc = 0; cc < 7; cc++) {
            double t = J[r] * J[cc];
#pragma unroll
            for (int k = 1; k < 7; k++) t += J[k * 7 + r] * J[k * 7 + cc];
            acc[cc] += t;
        }
        double t = J[r] * (-er[0]);
#pragma unroll
        for (int k = 1; k < 7; k++) t += J[k * 7 + r] * (-er[k]);
        acc[7] += t;
    }
#pragma unroll
    for (int cc = 0; cc < 7; cc++) D.Hd[(size_t)col * 49 + r * 7 + cc] = acc[cc];
    D.b[(size_t)col * 7 + r] = acc[7];
}

// the off-diagonal part: row a of the block of pair item / 7, (row vertex)^T (column vertex), over the pair's edges in ascending
// input index
__global__ __launch_bounds__(EG_THREADS) void k_eg_offdiag(EgDev D) {
    const int item = blockIdx.x * EG_THREADS + threadIdx.x;
    const int o = item / 7, a = item % 7;
    if (o >= D.noff) return;
    const int vr = D.vtxOfCol[D.oRow[o]];
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = D.oStart[o]; i < D.oStart[o + 1]; i++) {
        const int e = D.oEdges[i];
        const int sr = D.edges[e].i == vr ? 0 : 1;
        const double *Jr = D.jac + ((size_t)e * 2 + sr) * 49, *Jc = D.jac + ((size_t)e * 2 + (sr ^ 1)) * 49;
#pragma unroll
        for (int bb = 0; bb < 7; bb++) {
            double t = Jr[a] * Jc[bb];
#pragma unroll
            for (int k = 1; k < 7; k++) t += Jr[k * 7 + a] * Jc[k * 7 + bb];
            acc[bb] += t;
        }
    }
#pragma unroll
    for (int bb = 0; bb < 7; bb++) D.Hoff[(size_t)o * 49 + a * 7 + bb] = acc[bb];
}

// a trial: Hpp + lambda I into the factor's blocks (a fill block starts at zero), b into x, ok = 1
__global__ __launch_bounds__(EG_THREADS) void k_eg_assemble(EgDev D, double lambda) {
    const int item = blockIdx.x * EG_THREADS + threadIdx.x;
    if (item == 0) D.rec->ok = 1;
    if (item < D.nf * 7) D.x[item] = D.b[item];
    const int blk = item / 49, en = item % 49;
    if (blk >= D.nblk) return;
    const int r = D.blkRow[blk], cc = D.blkCol[blk], src = D.blkSrc[blk];
    double v = 0.0;
    if (r == cc) {
        v = D.Hd[(size_t)cc * 49 + en];
        if (en / 7 == en % 7) v += lambda;
    } else if (src >= 0) v = D.Hoff[(size_t)src * 49 + en];
    D.L[(size_t)blk * 49 + en] = v;
}

// One column of the block LDL^T, left-looking, one workgroup: (1) every entry of the column's blocks takes its updates
// -(L(r,k) D_k) L(c,k)^T in ascending k; (2) thread 0 factorises the diagonal block (unit lower L, the pivots on its diagonal); a
// zero, negative or non-finite pivot sets ok = 0 and goes on with 1.0 so that nothing else turns non-finite; (3) every row of every
// block below solves against L_cc^T and the pivots.  The columns of one launch are one level of the elimination tree.
__global__ __launch_bounds__(EG_THREADS) void k_eg_factor(EgDev D, int first) {
    __shared__ double Dg[49];
    const int c = D.lvlCols[first + blockIdx.x], b0 = D.colStart[c], nb = D.colStart[c + 1] - b0;
    for (int t = threadIdx.x; t < nb * 49; t += EG_THREADS) {
        const int blk = b0 + t / 49, a = (t % 49) / 7, bb = t % 7;
        double v = D.L[(size_t)blk * 49 + a * 7 + bb];
        for (int u = D.updStart[blk]; u < D.updStart[blk + 1]; u++) {
            const double *La = D.L + (size_t)D.updA[u] * 49 + a * 7, *Lb = D.L + (size_t)D.updB[u] * 49 + bb * 7, *Dk = D.L + (size_t)D.updD[u] * 49;
#pragma unroll
            for (int m = 0; m < 7; m++) v -= (La[m] * Dk[m * 8]) * Lb[m];
        }
        D.L[(size_t)blk * 49 + a * 7 + bb] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double *A = D.L + (size_t)b0 * 49;
        int bad = 0;
        for (int j = 0; j < 7; j++) {
            double v = A[j * 8];
            for (int m = 0; m < j; m++) v -= (Dg[j * 7 + m] * Dg[m * 8]) * Dg[j * 7 + m];
            if (!(v > 0.0) || !(v <= DBL_MAX)) { bad = 1; v = 1.0; }
            Dg[j * 8] = v;
            for (int i = j + 1; i < 7; i++) {
                double w = A[i * 7 + j];
                for (int m = 0; m < j; m++) w -= (Dg[i * 7 + m] * Dg[m * 8]) * Dg[j * 7 + m];
                Dg[i * 7 + j] = w / v;
            }
        }
        for (int j = 0; j < 7; j++)
            for (int i = j; i < 7; i++) A[i * 7 + j] = Dg[i * 7 + j];
        if (bad) D.rec->ok = 0;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < (nb - 1) * 7; t += EG_THREADS) {
        double *row = D.L + (size_t)(b0 + 1 + t / 7) * 49 + (t % 7) * 7;
        double xr[7];
#pragma unroll
        for (int bb = 0; bb < 7; bb++) {
            double v = row[bb];
#pragma unroll
            for (int m = 0; m < 7; m++)
                if (m < bb) v -= (xr[m] * Dg[m * 8]) * Dg[bb * 7 + m];
            xr[bb] = v / Dg[bb * 8];
        }
#pragma unroll
        for (int bb = 0; bb < 7; bb++) row[bb] = xr[bb];
    }
}

// L y = b, one thread per column of the level: the blocks (c, k) of the row in ascending k, then the unit lower diagonal block
__global__ __launch_bounds__(EG_THREADS) void k_eg_forward(EgDev D, int first, int n) {
    const int i = blockIdx.x * EG_THREADS + threadIdx.x;
    if (i >= n) return;
    const int c = D.lvlCols[first + i];
    double y[7];
#pragma unroll
    for (int a = 0; a < 7; a++) y[a] = D.x[c * 7 + a];
    for (int u = D.rowStart[c]; u < D.rowStart[c + 1]; u++) {
        const int blk = D.rowBlk[u];
        const double *Lb = D.L + (size_t)blk * 49, *yk = D.x + D.blkCol[blk] * 7;
#pragma unroll
        for (int a = 0; a < 7; a++)
#pragma unroll
            for (int m = 0; m < 7; m++) y[a] -= Lb[a * 7 + m] * yk[m];
    }
    const double *Lc = D.L + (size_t)D.colStart[c] * 49;
#pragma unroll
    for (int a = 1; a < 7; a++)
#pragma unroll
        for (int m = 0; m < 7; m++)
            if (m < a) y[a] -= Lc[a * 7 + m] * y[m];
#pragma unroll
    for (int a = 0; a < 7; a++) D.x[c * 7 + a] = y[a];
}

// D L^T x = y, one thread per column of the level (the levels run downwards): y / pivot, the blocks (r, c) below in ascending r,
// then the diagonal block's transpose
__global__ __launch_bounds__(EG_THREADS) void k_eg_backward(EgDev D, int first, int n) {
    const int i = blockIdx.x * EG_THREADS + threadIdx.x;
    if (i >= n) return;
    const int c = D.lvlCols[first + i], b0 = D.colStart[c];
    const double *Lc = D.L + (size_t)b0 * 49;
    double x[7];
#pragma unroll
    for (int a = 0; a < 7; a++) x[a] = D.x[c * 7 + a] / Lc[a * 8];
    for (int blk = b0 + 1; blk < D.colStart[c + 1]; blk++) {
        const double *Lb = D.L + (size_t)blk * 49, *xr = D.x + D.blkRow[blk] * 7;
#pragma unroll
        for (int a = 0; a < 7; a++)
#pragma unroll
            for (int m = 0; m < 7; m++) x[a] -= Lb[m * 7 + a] * xr[m];
    }
#pragma unroll
    for (int a = 5; a >= 0; a--)
#pragma unroll
        for (int m = 6; m >= 0; m--)
            if (m > a) x[a] -= Lc[m * 7 + a] * x[m];
#pragma unroll
    for (int a = 0; a < 7; a++) D.x[c * 7 + a] = x[a];
}

// The trial estimates from the current ones: oplusImpl, exp(x) * estimate, for a vertex with a column after a good solve, a copy
// otherwise.  Each workgroup leaves its share of computeScale: sum x (lambda x + b).
__global__ __launch_bounds__(EG_THREADS) void k_eg_update(EgDev D, int c, double lambda) {
    __shared__ double part[EG_WAVES];
    const int v = blockIdx.x * EG_THREADS + threadIdx.x;
    double sc = 0.0;
    if (v < D.N) {
        EgS3 S = D.est[c][v];
        const int col = D.colOf[v];
        if (col >= 0 && D.rec->ok) {
            double x[7];
#pragma unroll
            for (int j = 0; j < 7; j++) x[j] = D.x[col * 7 + j];
            if (D.fixScale) x[6] = 0.0;
#pragma unroll
            for (int j = 0; j < 7; j++) sc += x[j] * (lambda * x[j] + D.b[col * 7 + j]);
            S = sim3_mul(sim3_exp(x), S);
        }
        D.est[c ^ 1][v] = S;
    }
    sc = block_sum<EG_LANES, EG_WAVES>(sc, part);
    if (threadIdx.x == 0) D.partScale[blockIdx.x] = sc;
}

// activeChi2 from the partial sums (lin: of a linearisation, else of a trial, with computeScale)
__global__ __launch_bounds__(EG_THREADS) void k_eg_reduce(EgDev D, int nbE, int nbS, int lin) {
    __shared__ double part[2][EG_WAVES];
    double a1 = 0.0, a2 = 0.0;
    for (int i = threadIdx.x; i < nbE; i += EG_THREADS) a1 += D.partChi[i];
    for (int i = threadIdx.x; i < nbS; i += EG_THREADS) a2 += D.partScale[i];
    a1 = block_sum<EG_LANES, EG_WAVES>(a1, part[0]);
    a2 = block_sum<EG_LANES, EG_WAVES>(a2, part[1]);
    if (threadIdx.x == 0) {
        if (lin) D.rec->linChi = a1;
        else { D.rec->tmpChi = a1; D.rec->scale = a2; }
    }
}

// :994-1011: [R, t / s] of every estimate, a fixed vertex's too; :1018-1048: correctedSwr.map(Srw.map(P)) with Srw the vScw entry
__global__ __launch_bounds__(EG_THREADS) void k_eg_out(EgDev D, int c) {
    const int i = blockIdx.x * EG_THREADS + threadIdx.x;
    if (i < D.N) {
        const EgS3 S = D.est[c][i];
        double R[9];
        quat_to_R(S.q, R);
        const double is = 1. / S.s;
        float *to = D.outT + (size_t)i * 16;
        for (int r = 0; r < 3; r++) {
            for (int cc = 0; cc < 3; cc++) to[r * 4 + cc] = (float)R[r * 3 + cc];
            to[r * 4 + 3] = (float)(S.t[r] * is);
        }
        to[12] = 0.f; to[13] = 0.f; to[14] = 0.f; to[15] = 1.f;
        double *eo = D.outE + (size_t)i * 8;
        eo[0] = S.q[0]; eo[1] = S.q[1]; eo[2] = S.q[2]; eo[3] = S.q[3]; eo[4] = S.t[0]; eo[5] = S.t[1]; eo[6] = S.t[2]; eo[7] = S.s;
    }
    if (i < D.P) {
        const orbg_point_t p = D.pts[i];
        const double X[3] = {(double)p.x, (double)p.y, (double)p.z};
        double Xr[3], Xw[3];
        sim3_map(D.vtx[p.ref].Scw, X, Xr);
        sim3_map(sim3_inverse(D.est[c][p.ref]), Xr, Xw);
        for (int k = 0; k < 3; k++) D.outP[(size_t)i * 3 + k] = (float)Xw[k];
    }
}

// ------------------------------------------------------------------------------------
// the argument checks, before a device is touched
static inline bool eg_finite(double v) { return v >= -DBL_MAX && v <= DBL_MAX; }
static inline bool eg_sim3_ok(const orbg_sim3_t &S) {
    bool ok = eg_finite(S.s) && S.s > 0.0;
    for (int k = 0; k < 4; k++) ok = ok && eg_finite(S.q[k]);
    for (int k = 0; k < 3; k++) ok = ok && eg_finite(S.t[k]);
    return ok;
}
static int eg_check(const char *fn, const orbg_vertex_t *vtx, int N, const orbg_edge_t *edges, int E, const orbg_point_t *pts, int P, int iterations,
                    const float *Tcw_out, const float *pts_out) {
    if (N < 0 || E < 0 || P < 0 || (N > 0 && (!vtx || !Tcw_out)) || (E > 0 && !edges) || (P > 0 && (!pts || !pts_out))) {
        orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG;
    }
    if (iterations < 0 || iterations > ORBG_MAX_ITERATIONS) { orbx_set_error("%s: iterations outside 0..%d", fn, ORBG_MAX_ITERATIONS); return ORBX_ERR_ARG; }
    for (int v = 0; v < N; v++)
        if (!eg_sim3_ok(vtx[v].Scw) || (vtx[v].has_nc && !eg_sim3_ok(vtx[v].Snc))) {
            orbx_set_error("%s: vertex %d is not finite or its scale is not positive", fn, v); return ORBX_ERR_ARG;
        }
    for (int e = 0; e < E; e++) {
        const orbg_edge_t &ed = edges[e];
        if (ed.i < 0 || ed.i >= N || ed.j < 0 || ed.j >= N || ed.i == ed.j || (ed.kind != 0 && ed.kind != 1)) {
            orbx_set_error("%s: edge %d joins vertices %d and %d with kind %d", fn, e, ed.i, ed.j, ed.kind); return ORBX_ERR_ARG;
        }
    }
    for (int p = 0; p < P; p++) {
        const orbg_point_t &q = pts[p];
        if (q.ref < 0 || q.ref >= N || !eg_finite((double)q.x) || !eg_finite((double)q.y) || !eg_finite((double)q.z)) {
            orbx_set_error("%s: point %d is not finite or names vertex %d", fn, p, q.ref); return ORBX_ERR_ARG;
        }
    }
    return ORBX_OK;
}

// ------------------------------------------------------------------------------------
// The symbolic half, once per call.  ORDERING: the natural one - the free vertices (not fixed, with an edge) in ascending vertex
// index; it keeps the band of a covisibility graph, a loop becomes a few full rows at the end, and the elimination tree of a band
// is a chain (one column per level).
struct EgSym {
    int nf = 0, nblk = 0, noff = 0, nlev = 0;
    std::vector<int32_t> colOf, vtxOfCol, vStart, vEdges, oRow, oCol, oStart, oEdges, colStart, blkRow, blkCol, blkSrc, updStart, updA, updB, updD,
        rowStart, rowBlk, lvlStart, lvlCols;
};
static EgSym eg_symbolic(const orbg_vertex_t *vtx, int N, const orbg_edge_t *edges, int E) {
    EgSym S;
    S.colOf.assign((size_t)N, -1);
    std::vector<uint8_t> has((size_t)N, 0);
    for (int e = 0; e < E; e++) { has[edges[e].i] = 1; has[edges[e].j] = 1; }
    for (int v = 0; v < N; v++)
        if (has[v] && !vtx[v].fixed) { S.colOf[v] = S.nf++; S.vtxOfCol.push_back(v); }
    const int nf = S.nf;
    // CSR by column, and the pairs
    S.vStart.assign((size_t)nf + 1, 0);
    std::vector<uint64_t> pairs;   // (column column, row column, edge): sorted, a pair's edges come out in ascending input index
    std::vector<std::vector<int32_t>> st((size_t)nf);   // per column: the rows below the diagonal
    for (int e = 0; e < E; e++) {
        const int ci = S.colOf[edges[e].i], cj = S.colOf[edges[e].j];
        if (ci >= 0) S.vStart[ci + 1]++;
        if (cj >= 0) S.vStart[cj + 1]++;
        if (ci >= 0 && cj >= 0) st[std::min(ci, cj)].push_back(std::max(ci, cj));
    }
    for (int c = 0; c < nf; c++) S.vStart[c + 1] += S.vStart[c];
    S.vEdges.resize((size_t)S.vStart[nf]);
    {
        std::vector<int32_t> nx(S.vStart.begin(), S.vStart.end() - 1);
        for (int e = 0; e < E; e++) {
            const int ci = S.colOf[edges[e].i], cj = S.colOf[edges[e].j];
            if (ci >= 0) S.vEdges[nx[ci]++] = e;
            if (cj >= 0) S.vEdges[nx[cj]++] = e;
        }
    }
    // the pairs column by column, rows ascending: (column, row) lexicographic
    std::vector<std::vector<int32_t>> pairOf((size_t)nf);   // per column: pair index of every distinct row, aligned with the deduplicated st[c]
    for (int c = 0; c < nf; c++) { std::sort(st[c].begin(), st[c].end()); st[c].erase(std::unique(st[c].begin(), st[c].end()), st[c].end()); }
    std::vector<int32_t> pairBase((size_t)nf + 1, 0);
    for (int c = 0; c < nf; c++) pairBase[c + 1] = pairBase[c] + (int32_t)st[c].size();
    S.noff = pairBase[nf];
    S.oRow.resize((size_t)S.noff); S.oCol.resize((size_t)S.noff); S.oStart.assign((size_t)S.noff + 1, 0);
    for (int c = 0; c < nf; c++)
        for (size_t k = 0; k < st[c].size(); k++) { S.oCol[pairBase[c] + k] = c; S.oRow[pairBase[c] + k] = st[c][k]; }
    auto pair_index = [&](int c, int r) { return pairBase[c] + (int)(std::lower_bound(st[c].begin(), st[c].end(), r) - st[c].begin()); };
    for (int e = 0; e < E; e++) {
        const int ci = S.colOf[edges[e].i], cj = S.colOf[edges[e].j];
        if (ci >= 0 && cj >= 0) S.oStart[pair_index(std::min(ci, cj), std::max(ci, cj)) + 1]++;
    }
    for (int o = 0; o < S.noff; o++) S.oStart[o + 1] += S.oStart[o];
    S.oEdges.resize((size_t)S.oStart[S.noff]);
    {
        std::vector<int32_t> nx(S.oStart.begin(), S.oStart.end() - 1);
        for (int e = 0; e < E; e++) {
            const int ci = S.colOf[edges[e].i], cj = S.colOf[edges[e].j];
            if (ci >= 0 && cj >= 0) S.oEdges[nx[pair_index(std::min(ci, cj), std::max(ci, cj))]++] = e;
        }
    }
    // the pattern of the factor: struct(c) = adj(c) + the structs of c's children without c; parent(c) = min struct(c)
    std::vector<std::vector<int32_t>> fs(st);
    std::vector<int32_t> parent((size_t)nf, -1), level((size_t)nf, 0);
    for (int c = 0; c < nf; c++) {
        std::sort(fs[c].begin(), fs[c].end());
        fs[c].erase(std::unique(fs[c].begin(), fs[c].end()), fs[c].end());
        if (fs[c].empty()) continue;
        const int p = fs[c][0];
        parent[c] = p;
        fs[p].insert(fs[p].end(), fs[c].begin() + 1, fs[c].end());   // p's own turn comes later (p > c): sorted and deduplicated then
        level[p] = std::max(level[p], level[c] + 1);
    }
    S.colStart.assign((size_t)nf + 1, 0);
    for (int c = 0; c < nf; c++) S.colStart[c + 1] = S.colStart[c] + 1 + (int32_t)fs[c].size();
    S.nblk = S.colStart[nf];
    S.blkRow.resize((size_t)S.nblk); S.blkCol.resize((size_t)S.nblk); S.blkSrc.assign((size_t)S.nblk, -1);
    std::vector<std::vector<int32_t>> rows((size_t)nf);   // per column c: the blocks (c, k), k ascending
    for (int c = 0; c < nf; c++) {
        int b = S.colStart[c];
        S.blkRow[b] = c; S.blkCol[b] = c;
        for (size_t k = 0; k < fs[c].size(); k++) {
            b = S.colStart[c] + 1 + (int)k;
            S.blkRow[b] = fs[c][k]; S.blkCol[b] = c;
            if (std::binary_search(st[c].begin(), st[c].end(), fs[c][k])) S.blkSrc[b] = pair_index(c, fs[c][k]);
            rows[fs[c][k]].push_back(b);
        }
    }
    S.rowStart.assign((size_t)nf + 1, 0);
    for (int c = 0; c < nf; c++) { S.rowStart[c + 1] = S.rowStart[c] + (int32_t)rows[c].size(); S.rowBlk.insert(S.rowBlk.end(), rows[c].begin(), rows[c].end()); }
    // the updates of block (r, c): every k < c whose column holds both row c and row r
    S.updStart.assign((size_t)S.nblk + 1, 0);
    for (int c = 0; c < nf; c++)
        for (int b = S.colStart[c]; b < S.colStart[c + 1]; b++) {
            const int r = S.blkRow[b];
            for (int32_t bc : rows[c]) {
                const int k = S.blkCol[bc];
                int ba = bc;
                if (r != c) {
                    const auto it = std::lower_bound(fs[k].begin(), fs[k].end(), r);
                    if (it == fs[k].end() || *it != r) continue;
                    ba = S.colStart[k] + 1 + (int)(it - fs[k].begin());
                }
                S.updA.push_back(ba); S.updB.push_back(bc); S.updD.push_back(S.colStart[k]);
            }
            S.updStart[b + 1] = (int32_t)S.updA.size();
        }
    for (int c = 0; c < nf; c++) S.nlev = std::max(S.nlev, level[c] + 1);
    S.lvlStart.assign((size_t)S.nlev + 1, 0);
    for (int c = 0; c < nf; c++) S.lvlStart[level[c] + 1]++;
    for (int l = 0; l < S.nlev; l++) S.lvlStart[l + 1] += S.lvlStart[l];
    S.lvlCols.resize((size_t)nf);
    {
        std::vector<int32_t> nx(S.lvlStart.begin(), S.lvlStart.end() - (S.nlev ? 1 : 0));
        for (int c = 0; c < nf; c++) S.lvlCols[nx[level[c]]++] = c;
    }
    return S;
}

// ------------------------------------------------------------------------------------
// The memory of one call.  The library: a device block, its pinned mirror and a stream (this thread's StagePair).  The lockstep
// program: one host block that is both, a launch is a loop over blockIdx.x.
struct EgMem {
    uint8_t *d, *h;
#ifdef ORBX_EG_HOST
    int push(size_t, size_t) { return ORBX_OK; }
    int fetch(size_t, size_t) { return ORBX_OK; }
#else
    hipStream_t st;
    int push(size_t off, size_t bytes) { ORBX_HIP(hipMemcpyAsync(d + off, h + off, bytes, hipMemcpyHostToDevice, st)); return ORBX_OK; }
    int fetch(size_t off, size_t bytes) {   // the ONE synchronisation of a trial
        ORBX_HIP(hipMemcpyAsync(h + off, d + off, bytes, hipMemcpyDeviceToHost, st));
        ORBX_HIP(hipStreamSynchronize(st));
        return ORBX_OK;
    }
#endif
};
#ifdef ORBX_EG_HOST
#define EG_LAUNCH(kern, grid, ...) do { for (int b_ = 0; b_ < (int)(grid); b_++) { blockIdx.x = b_; kern(__VA_ARGS__); } blockIdx.x = 0; nlaunch++; } while (0)
#else
#define EG_LAUNCH(kern, grid, ...) do { hipLaunchKernelGGL(kern, dim3(grid), dim3(EG_THREADS), 0, M.st, __VA_ARGS__); ORBX_HIP(hipGetLastError()); nlaunch++; } while (0)
#endif
#define EG_TRY(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

#define EG_SYM_ARRAYS(X) X(colOf) X(vtxOfCol) X(vStart) X(vEdges) X(oRow) X(oCol) X(oStart) X(oEdges) X(colStart) X(blkRow) X(blkCol) X(blkSrc) \
    X(updStart) X(updA) X(updB) X(updD) X(rowStart) X(rowBlk) X(lvlCols)
struct EgLayout {
    size_t oVtx, oEdges, oPts;
#define X(a) size_t o_##a;
    EG_SYM_ARRAYS(X)
#undef X
    size_t inEnd, oRec, oOutT, oOutP, oOutE, outEnd;
    size_t oEst[2], oMeas, oErr, oJac, oHd, oB, oHoff, oL, oX, oPartChi, oPartScale, total;
    int nbLin, nbE, nbN, nbAll;
};
static inline int eg_blocks(long long n) { return (int)((n + EG_THREADS - 1) / EG_THREADS); }
static EgLayout eg_layout(const EgSym &S, int N, int E, int P) {
    EgLayout L;
    StagePlan pl;
    const size_t n1 = (size_t)(N > 0 ? N : 1), e1 = (size_t)(E > 0 ? E : 1), p1 = (size_t)(P > 0 ? P : 1), f1 = (size_t)(S.nf > 0 ? S.nf : 1);
    L.nbLin = eg_blocks((long long)E * EG_SLOTS); L.nbE = eg_blocks(E); L.nbN = eg_blocks(N);
    L.nbAll = eg_blocks(std::max(N, std::max(E, P)));
    // uploaded once
    L.oVtx = pl.take(n1 * sizeof(orbg_vertex_t)); L.oEdges = pl.take(e1 * sizeof(orbg_edge_t)); L.oPts = pl.take(p1 * sizeof(orbg_point_t));
#define X(a) L.o_##a = pl.take((S.a.size() + 1) * 4);
    EG_SYM_ARRAYS(X)
#undef X
    L.inEnd = pl.off;
    // downloaded per trial; downloaded at the end
    L.oRec = pl.take(sizeof(EgRec));
    L.oOutT = pl.take(n1 * 64); L.oOutP = pl.take(p1 * 12); L.oOutE = pl.take(n1 * 64);
    L.outEnd = pl.off;
    // device only
    for (int i = 0; i < 2; i++) L.oEst[i] = pl.take(n1 * sizeof(EgS3));
    L.oMeas = pl.take(e1 * sizeof(EgS3)); L.oErr = pl.take(e1 * 56); L.oJac = pl.take(e1 * 2 * 49 * 8);
    L.oHd = pl.take(f1 * 49 * 8); L.oB = pl.take(f1 * 56); L.oHoff = pl.take((size_t)(S.noff > 0 ? S.noff : 1) * 49 * 8);
    L.oL = pl.take((size_t)(S.nblk > 0 ? S.nblk : 1) * 49 * 8); L.oX = pl.take(f1 * 56);
    L.oPartChi = pl.take((size_t)(L.nbLin > 0 ? L.nbLin : 1) * 8); L.oPartScale = pl.take((size_t)(L.nbN > 0 ? L.nbN : 1) * 8);
    L.total = pl.off;
    return L;
}

// the inputs and the symbolic arrays into the mirror
static void eg_stage(uint8_t *h, const EgLayout &L, const EgSym &S, const orbg_vertex_t *vtx, int N, const orbg_edge_t *edges, int E, const orbg_point_t *pts, int P) {
    if (N) memcpy(h + L.oVtx, vtx, (size_t)N * sizeof(orbg_vertex_t));
    if (E) memcpy(h + L.oEdges, edges, (size_t)E * sizeof(orbg_edge_t));
    if (P) memcpy(h + L.oPts, pts, (size_t)P * sizeof(orbg_point_t));
#define X(a) if (!S.a.empty()) memcpy(h + L.o_##a, S.a.data(), S.a.size() * 4);
    EG_SYM_ARRAYS(X)
#undef X
}

// optimize(iterations) (sparse_optimizer.cpp:376) over the Levenberg-Marquardt of optimization_algorithm_levenberg.cpp:61-164 with
// setUserLambdaInit(1e-16).  M.h holds the inputs on entry (eg_stage) and the outputs on return.  The loops are bounded:
// iterations x 10 trials.
static int eg_drive(EgMem M, const EgLayout &L, const EgSym &S, int N, int E, int P, int fixScale, int iterations, orbg_info_t *info) {
    EgDev D;
    uint8_t *d = M.d;
    D.N = N; D.E = E; D.P = P; D.nf = S.nf; D.nblk = S.nblk; D.noff = S.noff; D.fixScale = fixScale ? 1 : 0; D.pad = 0;
    D.vtx = (const orbg_vertex_t *)(d + L.oVtx); D.edges = (const orbg_edge_t *)(d + L.oEdges); D.pts = (const orbg_point_t *)(d + L.oPts);
#define X(a) D.a = (const int32_t *)(d + L.o_##a);
    EG_SYM_ARRAYS(X)
#undef X
    for (int i = 0; i < 2; i++) D.est[i] = (EgS3 *)(d + L.oEst[i]);
    D.meas = (EgS3 *)(d + L.oMeas); D.err = (double *)(d + L.oErr); D.jac = (double *)(d + L.oJac); D.Hd = (double *)(d + L.oHd);
    D.b = (double *)(d + L.oB); D.Hoff = (double *)(d + L.oHoff); D.L = (double *)(d + L.oL); D.x = (double *)(d + L.oX);
    D.partChi = (double *)(d + L.oPartChi); D.partScale = (double *)(d + L.oPartScale); D.rec = (EgRec *)(d + L.oRec);
    D.outT = (float *)(d + L.oOutT); D.outP = (float *)(d + L.oOutP); D.outE = (double *)(d + L.oOutE);
    const EgRec *hrec = (const EgRec *)(M.h + L.oRec);

    orbg_info_t inf;
    memset(&inf, 0, sizeof(inf));
    inf.free_vertices = S.nf; inf.blocks = S.nblk; inf.levels = S.nlev;
    int nlaunch = 0;
    EG_TRY(M.push(0, L.inEnd));
    if (L.nbAll) EG_LAUNCH(k_eg_init, L.nbAll, D);
    int c = 0;
    double lambda = 0.0, ni = 2.0, cur = 0.0;
    int nbad = 0, lastOk = 1;
    bool ok = true;
    // optimize(): no active edge or "0 vertices to optimize" -> no iteration
    for (int it = 0; it < iterations && ok && E > 0 && S.nf > 0; it++) {
        EG_LAUNCH(k_eg_edges<true>, L.nbLin, D, c);
        EG_LAUNCH(k_eg_vertex, eg_blocks((long long)S.nf * 7), D);
        if (S.noff) EG_LAUNCH(k_eg_offdiag, eg_blocks((long long)S.noff * 7), D);
        EG_LAUNCH(k_eg_reduce, 1, D, L.nbLin, 0, 1);
        if (it == 0) { lambda = 1e-16; ni = 2.0; nbad = 0; }   // computeLambdaInit: the user's value
        double iniChi = 0.0, rho = 0.0;
        int q = 0;
        do {
            EG_LAUNCH(k_eg_assemble, eg_blocks((long long)S.nblk * 49), D, lambda);
            for (int l = 0; l < S.nlev; l++) EG_LAUNCH(k_eg_factor, S.lvlStart[l + 1] - S.lvlStart[l], D, S.lvlStart[l]);
            for (int l = 0; l < S.nlev; l++) EG_LAUNCH(k_eg_forward, eg_blocks(S.lvlStart[l + 1] - S.lvlStart[l]), D, S.lvlStart[l], S.lvlStart[l + 1] - S.lvlStart[l]);
            for (int l = S.nlev - 1; l >= 0; l--) EG_LAUNCH(k_eg_backward, eg_blocks(S.lvlStart[l + 1] - S.lvlStart[l]), D, S.lvlStart[l], S.lvlStart[l + 1] - S.lvlStart[l]);
            EG_LAUNCH(k_eg_update, L.nbN, D, c, lambda);
            EG_LAUNCH(k_eg_edges<false>, L.nbE, D, c ^ 1);
            EG_LAUNCH(k_eg_reduce, 1, D, L.nbE, L.nbN, 0);
            EG_TRY(M.fetch(L.oRec, sizeof(EgRec)));
            if (q == 0) { cur = hrec->linChi; iniChi = cur; if (it == 0) inf.chi2_first = cur; }
            double tmp = hrec->tmpChi;
            lastOk = hrec->ok;
            if (!lastOk) tmp = DBL_MAX;
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
        } while (rho < 0.0 && q < EG_MAX_TRIALS);
        inf.trials_it[inf.iterations++] = q; inf.trials += q;
        if (q == EG_MAX_TRIALS || rho == 0.0) { ok = false; inf.end = !lastOk ? ORBG_END_SOLVER : q == EG_MAX_TRIALS ? ORBG_END_QMAX : ORBG_END_RHO0; continue; }
        if ((iniChi - cur) * 1e3 < iniChi) nbad++; else nbad = 0;   // the reference's own stop criterion
        if (nbad >= 3) { ok = false; inf.end = ORBG_END_NBAD; }
    }
    inf.chi2_last = cur;
    if (L.nbAll) EG_LAUNCH(k_eg_out, L.nbAll, D, c);
    inf.launches = nlaunch;
    EG_TRY(M.fetch(L.oOutT, L.outEnd - L.oOutT));
    if (info) *info = inf;
    return ORBX_OK;
}
static void eg_results(const uint8_t *h, const EgLayout &L, int N, int P, float *Tcw_out, float *pts_out, double *est_out) {
    if (N) memcpy(Tcw_out, h + L.oOutT, (size_t)N * 64);
    if (P) memcpy(pts_out, h + L.oOutP, (size_t)P * 12);
    if (est_out && N) memcpy(est_out, h + L.oOutE, (size_t)N * 64);
}

#ifndef ORBX_EG_HOST
// host side: this thread's staging pair (orbx_stage.h)
static thread_local StagePair g_eg;
void orbx_internal_release_essential_scratch() { g_eg.release(); }

extern "C" int orbg_optimize_essential_graph(const orbg_vertex_t *vertices, int N, const orbg_edge_t *edges, int E, const orbg_point_t *points, int P,
                                             int fix_scale, int iterations, float *Tcw_out16, float *pts_out3, double *est_out8, orbg_info_t *info,
                                             int device) {
    const int crc = eg_check("orbg_optimize_essential_graph", vertices, N, edges, E, points, P, iterations, Tcw_out16, pts_out3);
    if (crc) return crc;
    const EgSym S = eg_symbolic(vertices, N, edges, E);
    const EgLayout L = eg_layout(S, N, E, P);
    int rc = g_eg.reserve(device, L.total, (size_t)1 << 20);
    if (rc) return rc;
    EgMem M;
    M.d = g_eg.d; M.h = g_eg.h; M.st = g_eg.stream;
    eg_stage(M.h, L, S, vertices, N, edges, E, points, P);
    (void)hipGetLastError();
    rc = eg_drive(M, L, S, N, E, P, fix_scale, iterations, info);
    if (rc) { hipStreamSynchronize(M.st); return rc; }
    eg_results(M.h, L, N, P, Tcw_out16, pts_out3, est_out8);
    return ORBX_OK;
}
#endif   // ORBX_EG_HOST
