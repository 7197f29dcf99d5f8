// orbx_jacobi_eig.h — the eigen-decomposition of a symmetric float 4x4 for Sim3Solver (Horn's N matrix): a two-sided cyclic Jacobi
// in double, this library's own stand-in for cv::eigen.  DESIGN.md section 6 ("k_sim3_*") specifies it operation by operation;
// tests/sim3_ref.py is the same sequence in numpy.  Not pinned to OpenCV.  NOT the one-sided SVD of orbx_jacobi_svd.h: N is
// traceless, so its largest singular value may belong to its most negative eigenvalue.
//
// A = (double)N, V = I, thr = JE_EPS sqrt(sum of all 16 A[i][j]^2, row-major).  For every pair p < q in the order (0,1), (0,2),
// (0,3), (1,2), (1,3), (2,3):
//     g = A[p][q];  rotate iff |g| > thr                                        (false for NaN: nothing can spin)
//     theta = (A[q][q] - A[p][p]) / (2 g)
//     t = 1 / (|theta| + sqrt(theta theta + 1)), negated when theta < 0;  c = 1 / sqrt(t t + 1);  s = t c
//     A[p][p] -= t g;  A[q][q] += t g;  A[p][q] = A[q][p] = 0
//     the two k other than p, q ascending:  x = A[k][p], y = A[k][q];  A[k][p] = A[p][k] = c x - s y;  A[k][q] = A[q][k] = s x + c y
//     every row k of V:                     x = V[k][p], y = V[k][q];  V[k][p] = c x - s y;  V[k][q] = s x + c y
// until a sweep rotates nothing or JE_MAX_SWEEPS sweeps are done.  eval[k] = (float)A[j][j], evec row k = (float) column j of V,
// j taken by descending A[j][j] with a stable selection (of equal values the lower column first; NaN compares false and stays).
// The sign of an eigenvector is whatever the rotations leave.
#ifndef ORBX_JACOBI_EIG_H
#define ORBX_JACOBI_EIG_H
#include <float.h>
#include <math.h>

#define JE_MAX_SWEEPS 30
#define JE_EPS DBL_EPSILON

__device__ __forceinline__ void jacobi_eig4(const float *N, float *eval, float *evec) {
    double A[16], V[16], ss = 0.0;
    for (int k = 0; k < 16; k++) { A[k] = (double)N[k]; V[k] = (k % 5 == 0) ? 1.0 : 0.0; ss += A[k] * A[k]; }
    const double thr = JE_EPS * sqrt(ss);
    for (int sweep = 0; sweep < JE_MAX_SWEEPS; sweep++) {
        bool changed = false;
#pragma unroll
        for (int p = 0; p < 3; p++) {
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                const double g = A[p * 4 + q];
                if (fabs(g) > thr) {
                    changed = true;
                    const double theta = (A[q * 4 + q] - A[p * 4 + p]) / (2.0 * g);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    A[p * 4 + p] -= t * g;
                    A[q * 4 + q] += t * g;
                    A[p * 4 + q] = 0.0; A[q * 4 + p] = 0.0;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (k == p || k == q) continue;
                        const double x = A[k * 4 + p], y = A[k * 4 + q];
                        A[k * 4 + p] = c * x - s * y; A[p * 4 + k] = A[k * 4 + p];
                        A[k * 4 + q] = s * x + c * y; A[q * 4 + k] = A[k * 4 + q];
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const double x = V[k * 4 + p], y = V[k * 4 + q];
                        V[k * 4 + p] = c * x - s * y;
                        V[k * 4 + q] = s * x + c * y;
                    }
                }
            }
        }
        if (!changed) break;
    }
    unsigned used = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        int best = -1;
        double bv = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++)
            if (!(used >> j & 1) && (best < 0 || A[j * 5] > bv)) { best = j; bv = A[j * 5]; }
        used |= 1u << best;
        eval[k] = (float)bv;
#pragma unroll
        for (int r = 0; r < 4; r++) {     // column `best` of V without a dynamic index into the private array
            double v = V[r * 4];
            if (best == 1) v = V[r * 4 + 1];
            if (best == 2) v = V[r * 4 + 2];
            if (best == 3) v = V[r * 4 + 3];
            evec[k * 4 + r] = (float)v;
        }
    }
}

// jacobi_eig<N>: the same rotations on a symmetric double N x N held in memory (PnPsolver: the 12x12 MtM and the 3x3 PCA matrix;
// DESIGN.md section 6, "k_pnp_*"; tests/pnp_ref.py).  A is overwritten (its diagonal ends as the eigenvalues), V [N][N] is set to
// the identity and ends with the eigenvectors in its COLUMNS.  thr = JE_EPS sqrt(sum of all N N A[i][j]^2, row-major); pairs
// (p, q) in the cyclic order; g, A[p][p] and A[q][q] are read before anything of the pair is written.  The 2 N row updates of a
// pair - the N - 2 rows k of A, the two diagonal entries, the N rows of V - are independent, so with COOP the threads tid, tid + nth,
// .. of a workgroup share them (A and V in LDS, two barriers per pair) and leave the bytes one thread leaves.
template <int N, bool COOP>
__device__ __forceinline__ void jacobi_eig(double *A, double *V, int tid, int nth) {
    double ss = 0.0;
    for (int k = 0; k < N * N; k++) ss += A[k] * A[k];
    const double thr = JE_EPS * sqrt(ss);
    for (int k = tid; k < N * N; k += nth) V[k] = (k % (N + 1) == 0) ? 1.0 : 0.0;
    if (COOP) __syncthreads();
    for (int sweep = 0; sweep < JE_MAX_SWEEPS; sweep++) {
        bool changed = false;
        for (int p = 0; p < N - 1; p++) {
            for (int q = p + 1; q < N; q++) {
                const double g = A[p * N + q], app = A[p * N + p], aqq = A[q * N + q];
                if (COOP) __syncthreads();
                if (fabs(g) > thr) {
                    changed = true;
                    const double theta = (aqq - app) / (2.0 * g);
                    double t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
                    if (theta < 0.0) t = -t;
                    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                    for (int k = tid; k < 2 * N; k += nth) {
                        if (k == p) { A[p * N + p] = app - t * g; A[p * N + q] = 0.0; }
                        else if (k == q) { A[q * N + q] = aqq + t * g; A[q * N + p] = 0.0; }
                        else if (k < N) {
                            const double x = A[k * N + p], y = A[k * N + q];
                            A[k * N + p] = c * x - s * y; A[p * N + k] = A[k * N + p];
                            A[k * N + q] = s * x + c * y; A[q * N + k] = A[k * N + q];
                        } else {
                            const int r = k - N;
                            const double x = V[r * N + p], y = V[r * N + q];
                            V[r * N + p] = c * x - s * y;
                            V[r * N + q] = s * x + c * y;
                        }
                    }
                }
                if (COOP) __syncthreads();
            }
        }
        if (!changed) break;
    }
}

// the order cvSVD gives a symmetric positive semi-definite matrix: w[j] = |A[j][j]|, order[k] = the columns by descending w, a stable
// selection (of equal values the lower column first; NaN compares false and stays where it is)
template <int N>
__device__ __forceinline__ void jacobi_eig_order(const double *A, double *w, int *order) {
    for (int j = 0; j < N; j++) w[j] = fabs(A[j * N + j]);
    unsigned used = 0;
    for (int k = 0; k < N; k++) {
        int best = -1;
        for (int j = 0; j < N; j++)
            if (!(used >> j & 1) && (best < 0 || w[j] > w[best])) best = j;
        used |= 1u << best;
        order[k] = best;
    }
}
#endif
