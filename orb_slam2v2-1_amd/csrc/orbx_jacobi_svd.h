// orbx_jacobi_svd.h — one float singular value decomposition for the small dense solvers (Initializer today; PnPsolver and
// Sim3Solver can reuse it): Hestenes' one-sided Jacobi, cyclic order, a fixed bound on sweeps.  DESIGN.md section 6
// ("k_init_*") specifies it operation by operation; tests/init_ref.py is the same sequence in numpy.  Not pinned to OpenCV's SVD.
//
// The working array W holds M + N rows of N floats: rows 0..M-1 are A (overwritten by A V = U diag(w)), rows M..M+N-1 are V and
// start as the identity.  For every pair p < q in the order (0,1), (0,2) .. (N-2,N-1):
//     a = sum_i A[i][p]^2, b = sum_i A[i][q]^2, g = sum_i A[i][p] A[i][q]      in double, i ascending over the M rows of A
//     rotate iff |g| > JS_EPS sqrt(a b)                                        (false for NaN: nothing can spin)
//     g2 = 2 g, beta = a - b, gamma = sqrt(g2 g2 + beta beta)
//     beta < 0:  s = sqrt(((gamma - beta) 0.5) / gamma), c = g2 / ((gamma s) 2)
//     else:      c = sqrt((gamma + beta) / (gamma 2)),   s = g2 / ((gamma c) 2)
//     every row r of W, in float with cf = (float)c, sf = (float)s:  x = W[r][p], y = W[r][q];  W[r][p] = cf x + sf y;  W[r][q] = cf y - sf x
// until a sweep rotates nothing or JS_MAX_SWEEPS sweeps are done.  Rows are independent, so a workgroup may share them out
// (COOP: W in LDS, every thread computes the three sums itself, two barriers per pair) and get the bytes one thread gets.
#ifndef ORBX_JACOBI_SVD_H
#define ORBX_JACOBI_SVD_H
#include <float.h>
#include <math.h>

#define JS_MAX_SWEEPS 30
#define JS_EPS (2.0 * (double)FLT_EPSILON)

template <int M, int N, bool COOP>
__device__ __forceinline__ void jacobi_sweeps(float *W, int tid, int nth) {
    for (int sweep = 0; sweep < JS_MAX_SWEEPS; sweep++) {
        bool changed = false;
        for (int p = 0; p < N - 1; p++) {
            for (int q = p + 1; q < N; q++) {
                double a = 0.0, b = 0.0, g = 0.0;
                for (int i = 0; i < M; i++) {
                    const double x = (double)W[i * N + p], y = (double)W[i * N + q];
                    a += x * x; b += y * y; g += x * y;
                }
                if (COOP) __syncthreads();
                if (fabs(g) > JS_EPS * sqrt(a * b)) {
                    changed = true;
                    const double g2 = 2.0 * g, beta = a - b, gamma = sqrt(g2 * g2 + beta * beta);
                    double c, s;
                    if (beta < 0.0) {
                        s = sqrt(((gamma - beta) * 0.5) / gamma);
                        c = g2 / ((gamma * s) * 2.0);
                    } else {
                        c = sqrt((gamma + beta) / (gamma * 2.0));
                        s = g2 / ((gamma * c) * 2.0);
                    }
                    const float cf = (float)c, sf = (float)s;
                    for (int r = tid; r < M + N; r += nth) {
                        const float x = W[r * N + p], y = W[r * N + q];
                        W[r * N + p] = cf * x + sf * y;
                        W[r * N + q] = cf * y - sf * x;
                    }
                }
                if (COOP) __syncthreads();
            }
        }
        if (!changed) break;
    }
}

// w[j] = (float)sqrt(sum_i A[i][j]^2) (double sum, i ascending) of the rotated A; order[] = the columns by descending w, a stable
// selection (of equal values the lower column first; NaN compares false and stays where it is)
template <int M, int N>
__device__ __forceinline__ void jacobi_order(const float *W, float *w, int *order) {
    for (int j = 0; j < N; j++) {
        double a = 0.0;
        for (int i = 0; i < M; i++) { const double x = (double)W[i * N + j]; a += x * x; }
        w[j] = (float)sqrt(a);
    }
    unsigned used = 0;
    for (int k = 0; k < N; k++) {
        int best = -1;
        for (int j = 0; j < N; j++)
            if (!(used >> j & 1) && (best < 0 || w[j] > w[best])) best = j;
        used |= 1u << best;
        order[k] = best;
    }
}

// 3x3 (row-major): A = U diag(w) Vt, w descending.  Vt row k = column order[k] of V; U column k = (A V)[:, order[k]] / w[k] for
// k = 0, 1; U column 2 = U0 x U1, negated when its double dot product with (A V)[:, order[2]] is negative - defined also when w[2]
// is zero (an essential matrix), where that column carries the translation.
__device__ __forceinline__ void svd3(const float *A, float *w, float *U, float *Vt) {
    float W[18];
    for (int k = 0; k < 9; k++) { W[k] = A[k]; W[9 + k] = (k == 0 || k == 4 || k == 8) ? 1.f : 0.f; }
    jacobi_sweeps<3, 3, false>(W, 0, 1);
    float wu[3];
    int order[3];
    jacobi_order<3, 3>(W, wu, order);
    for (int k = 0; k < 3; k++) {
        w[k] = wu[order[k]];
        for (int c = 0; c < 3; c++) Vt[k * 3 + c] = W[9 + c * 3 + order[k]];
    }
    for (int k = 0; k < 2; k++)
        for (int i = 0; i < 3; i++) U[i * 3 + k] = W[i * 3 + order[k]] / w[k];
    float u2[3];
    u2[0] = U[3] * U[7] - U[6] * U[4];
    u2[1] = U[6] * U[1] - U[0] * U[7];
    u2[2] = U[0] * U[4] - U[3] * U[1];
    double d = 0.0;
    for (int i = 0; i < 3; i++) d += (double)u2[i] * (double)W[i * 3 + order[2]];
    for (int i = 0; i < 3; i++) U[i * 3 + 2] = d < 0.0 ? -u2[i] : u2[i];
}

// 4x4: the right singular vector of the smallest singular value (vt.row(3))
__device__ __forceinline__ void svd4_null(const float *A, float *x) {
    float W[32];
    for (int k = 0; k < 16; k++) { W[k] = A[k]; W[16 + k] = (k % 5 == 0) ? 1.f : 0.f; }
    jacobi_sweeps<4, 4, false>(W, 0, 1);
    float w[4];
    int order[4];
    jacobi_order<4, 4>(W, w, order);
    for (int c = 0; c < 4; c++) x[c] = W[16 + c * 4 + order[3]];
}

// ---- the double flavour (PnPsolver's cvInvert / cvSolve / cvSVD with CV_SVD; DESIGN.md section 6, "k_pnp_*"; tests/pnp_ref.py):
// the same sweeps with the rows of W rotated in double (c and s are not narrowed) and JSD_EPS in the place of JS_EPS.  One thread.
#define JSD_EPS (2.0 * DBL_EPSILON)

template <int M, int N>
__device__ __forceinline__ void jacobi_sweeps_d(double *W) {
    for (int sweep = 0; sweep < JS_MAX_SWEEPS; sweep++) {
        bool changed = false;
        for (int p = 0; p < N - 1; p++) {
            for (int q = p + 1; q < N; q++) {
                double a = 0.0, b = 0.0, g = 0.0;
                for (int i = 0; i < M; i++) {
                    const double x = W[i * N + p], y = W[i * N + q];
                    a += x * x; b += y * y; g += x * y;
                }
                if (fabs(g) > JSD_EPS * sqrt(a * b)) {
                    changed = true;
                    const double g2 = 2.0 * g, beta = a - b, gamma = sqrt(g2 * g2 + beta * beta);
                    double c, s;
                    if (beta < 0.0) {
                        s = sqrt(((gamma - beta) * 0.5) / gamma);
                        c = g2 / ((gamma * s) * 2.0);
                    } else {
                        c = sqrt((gamma + beta) / (gamma * 2.0));
                        s = g2 / ((gamma * c) * 2.0);
                    }
                    for (int r = 0; r < M + N; r++) {
                        const double x = W[r * N + p], y = W[r * N + q];
                        W[r * N + p] = c * x + s * y;
                        W[r * N + q] = c * y - s * x;
                    }
                }
            }
        }
        if (!changed) break;
    }
}

// W [M + N][N]: rows 0..M-1 hold A on entry, rows M.. are set to the identity here.  After the sweeps w[j] = sqrt(sum_i W[i][j]^2)
// (i ascending); returns the pseudo-inverse threshold 2 DBL_EPSILON (w[0] + w[1] + ..), summed in column order.
template <int M, int N>
__device__ __forceinline__ double jacobi_svd_d(double *W, double *w) {
    for (int k = 0; k < N * N; k++) W[M * N + k] = (k % (N + 1) == 0) ? 1.0 : 0.0;
    jacobi_sweeps_d<M, N>(W);
    double sum = 0.0;
    for (int j = 0; j < N; j++) {
        double a = 0.0;
        for (int i = 0; i < M; i++) { const double x = W[i * N + j]; a += x * x; }
        w[j] = sqrt(a);
        sum += w[j];
    }
    return (2.0 * DBL_EPSILON) * sum;
}

// x = V diag(1 / w[j] where w[j] > thr) U^T b, with U[:, j] w[j] = W[0..M-1][j]: x starts at zero; for j ascending with w[j] > thr
// (false for NaN: the column is left out), s = sum_i W[i][j] b[i] (i ascending), coef = (s / w[j]) / w[j], x[k] += V[k][j] coef.
// A column whose w is not above thr is LEFT OUT of the sum; no U column is ever formed for it.
template <int M, int N>
__device__ __forceinline__ void jacobi_backsub_d(const double *W, const double *w, double thr, const double *b, double *x) {
    for (int k = 0; k < N; k++) x[k] = 0.0;
    for (int j = 0; j < N; j++) {
        if (!(w[j] > thr)) continue;
        double s = 0.0;
        for (int i = 0; i < M; i++) s += W[i * N + j] * b[i];
        const double coef = (s / w[j]) / w[j];
        for (int k = 0; k < N; k++) x[k] += W[(M + k) * N + j] * coef;
    }
}

// 3x3 (row-major) in double: A = U diag(w) V^T as svd3 above gives it, V NOT transposed (V[i][k] = component i of the k-th right
// vector): U columns 0, 1 divided by w, column 2 the cross product with the sign of its dot product with (A V)[:, order[2]].
// W: 18 doubles of work space.
__device__ __forceinline__ void svd3_d(const double *A, double *W, double *U, double *V) {
    for (int k = 0; k < 9; k++) { W[k] = A[k]; W[9 + k] = (k % 4 == 0) ? 1.0 : 0.0; }
    jacobi_sweeps_d<3, 3>(W);
    double w[3];
    for (int j = 0; j < 3; j++) {
        double a = 0.0;
        for (int i = 0; i < 3; i++) { const double x = W[i * 3 + j]; a += x * x; }
        w[j] = sqrt(a);
    }
    int order[3];
    unsigned used = 0;
#pragma unroll
    for (int k = 0; k < 3; k++) {     // the columns by descending w, the stable selection of jacobi_order
        int best = -1;
#pragma unroll
        for (int j = 0; j < 3; j++)
            if (!(used >> j & 1) && (best < 0 || w[j] > w[best])) best = j;
        used |= 1u << best;
        order[k] = best;
    }
    const int o0 = order[0], o1 = order[1], o2 = order[2];
    const double wo0 = w[o0], wo1 = w[o1];
    for (int i = 0; i < 3; i++) {
        V[i * 3] = W[9 + i * 3 + o0]; V[i * 3 + 1] = W[9 + i * 3 + o1]; V[i * 3 + 2] = W[9 + i * 3 + o2];
        U[i * 3] = W[i * 3 + o0] / wo0; U[i * 3 + 1] = W[i * 3 + o1] / wo1;
    }
    double u2[3];
    u2[0] = U[3] * U[7] - U[6] * U[4];
    u2[1] = U[6] * U[1] - U[0] * U[7];
    u2[2] = U[0] * U[4] - U[3] * U[1];
    double d = 0.0;
    for (int i = 0; i < 3; i++) d += u2[i] * W[i * 3 + o2];
    for (int i = 0; i < 3; i++) U[i * 3 + 2] = d < 0.0 ? -u2[i] : u2[i];
}
#endif
