// orbx_cvmath.h — OpenCV's small-matrix arithmetic on CV_32F as the reference's cv::Mat expressions evaluate it: the terms widened
// to double, summed left to right, scaled or shifted in double, narrowed to float ONCE.  Every function here is a bit-parity
// obligation against the OpenCV call its comment names; tests/init_ref.py and tests/sim3_ref.py restate the
// same trees in numpy.  An expression whose tree differs (a product after the sum, a float square) stays where it is used, with
// its comment.  Matrices are row-major; ld* is the distance between rows (3: a 3x3, 4: the top rows of a 4x4).
// No HIP header: tests/cpp/*_lockstep.cc compile this as plain C++.
#pragma once
#include <math.h>
#ifndef __host__   // plain C++ (the lockstep programs): host code is all there is
#define __host__
#endif
// __host__ too: orbl_compute_f12 and orbl_baseline_ok (orbx_newpoints.hip) are host code

// cv::gemm, d = alpha * a * b (BT: a * b.t(), GEMM_2_T) on 3x3: ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j) * alpha
template <bool BT = false>
__host__ __device__ __forceinline__ void gemm33(const float *a, const float *b, float *d, double alpha = 1.0) {
    const int bk = BT ? 1 : 3, bj = BT ? 3 : 1;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            d[i * 3 + j] = (float)((((double)a[i * 3] * (double)b[j * bj] + (double)a[i * 3 + 1] * (double)b[bk + j * bj]) + (double)a[i * 3 + 2] * (double)b[2 * bk + j * bj]) * alpha);
}
// cv::gemm, d = a * b on 4x4 (the poses' Tiw * Twc): (((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j) + a_i3 b_3j).  d may be neither a nor b
__host__ __device__ __forceinline__ void gemm44(const float *a, const float *b, float *d) {
    for (int i = 0; i < 4; i++)
        for (int j = 0; j < 4; j++)
            d[i * 4 + j] = (float)((((double)a[i * 4] * (double)b[j] + (double)a[i * 4 + 1] * (double)b[4 + j]) + (double)a[i * 4 + 2] * (double)b[8 + j]) + (double)a[i * 4 + 3] * (double)b[12 + j]);
}
// cv::gemm, d = alpha * a * x on a 3-vector: ((a_i0 x_0 + a_i1 x_1) + a_i2 x_2) * alpha
__host__ __device__ __forceinline__ void gemv3(const float *a, const float *x, float *d, double alpha = 1.0, int lda = 3, int ldd = 1) {
    for (int i = 0; i < 3; i++)
        d[i * ldd] = (float)((((double)a[i * lda] * (double)x[0] + (double)a[i * lda + 1] * (double)x[1]) + (double)a[i * lda + 2] * (double)x[2]) * alpha);
}
// cv::gemm with an added matrix, d = a * x + c on a 3-vector (GEMM expression a * x + c, alpha = beta = 1): ((a_i0 x_0 + a_i1 x_1) + a_i2 x_2) + c_i
__host__ __device__ __forceinline__ void gemv3_add(const float *a, const float *x, const float *c, float *d, int lda = 3) {
    for (int i = 0; i < 3; i++)
        d[i] = (float)((((double)a[i * lda] * (double)x[0] + (double)a[i * lda + 1] * (double)x[1]) + (double)a[i * lda + 2] * (double)x[2]) + (double)c[i]);
}
// cv::Mat::dot of a CV_32F row with a 3-vector, plus a float: (float)(((r_0 x_0 + r_1 x_1) + r_2 x_2) + t), the dot product a double
__host__ __device__ __forceinline__ float dot3_add(const float *r, const float *x, float t) {
    return (float)((((double)r[0] * (double)x[0] + (double)r[1] * (double)x[1]) + (double)r[2] * (double)x[2]) + (double)t);
}
// cv::Mat::t() of a 3x3 inside a matrix whose rows are lda apart: exact
__host__ __device__ __forceinline__ void transpose33(const float *a, float *d, int lda = 3) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) d[i * 3 + j] = a[j * lda + i];
}
// cv::determinant on 3x3 CV_32F: the cofactor expansion along row 0, in double
__host__ __device__ __forceinline__ double det3(const float *m) {
#define M_(i, j) (double)m[3 * (i) + (j)]
    return M_(0, 0) * (M_(1, 1) * M_(2, 2) - M_(1, 2) * M_(2, 1)) - M_(0, 1) * (M_(1, 0) * M_(2, 2) - M_(1, 2) * M_(2, 0)) +
           M_(0, 2) * (M_(1, 0) * M_(2, 1) - M_(1, 1) * M_(2, 0));
}
// cv::invert(DECOMP_LU) on 3x3 CV_32F: det3 in double, d = 1./d, adjugate x d narrowed; singular: the zero matrix
__host__ __device__ __forceinline__ void invert33(const float *m, float *t) {
    double d = det3(m);
    if (d == 0.0) { for (int k = 0; k < 9; k++) t[k] = 0.f; return; }
    d = 1. / d;
    t[0] = (float)((M_(1, 1) * M_(2, 2) - M_(1, 2) * M_(2, 1)) * d);
    t[1] = (float)((M_(0, 2) * M_(2, 1) - M_(0, 1) * M_(2, 2)) * d);
    t[2] = (float)((M_(0, 1) * M_(1, 2) - M_(0, 2) * M_(1, 1)) * d);
    t[3] = (float)((M_(1, 2) * M_(2, 0) - M_(1, 0) * M_(2, 2)) * d);
    t[4] = (float)((M_(0, 0) * M_(2, 2) - M_(0, 2) * M_(2, 0)) * d);
    t[5] = (float)((M_(0, 2) * M_(1, 0) - M_(0, 0) * M_(1, 2)) * d);
    t[6] = (float)((M_(1, 0) * M_(2, 1) - M_(1, 1) * M_(2, 0)) * d);
    t[7] = (float)((M_(0, 1) * M_(2, 0) - M_(0, 0) * M_(2, 1)) * d);
    t[8] = (float)((M_(0, 0) * M_(1, 1) - M_(0, 1) * M_(1, 0)) * d);
#undef M_
}
// cv::norm(NORM_L2) on a CV_32F 3-vector: (v_0^2 + v_1^2) + v_2^2 in double, double sqrt
__host__ __device__ __forceinline__ double norm3(const float *v) {
    return sqrt(((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1]) + (double)v[2] * (double)v[2]);
}
// the pinhole image of a camera point in float, as Sim3Solver::FromCameraToImage and the tail of Project write it
// (src/Sim3Solver.cc:397-401, :417-421): invz = 1 / z, no guard on z; K = fx fy cx cy
__host__ __device__ __forceinline__ void pinhole_image(const float *P, const float *K, float *uv) {
    const float invz = 1 / P[2];
    const float x = P[0] * invz, y = P[1] * invz;
    uv[0] = K[0] * x + K[2];
    uv[1] = K[1] * y + K[3];
}
