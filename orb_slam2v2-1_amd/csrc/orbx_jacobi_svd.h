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
#endif
