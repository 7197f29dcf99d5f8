// orbx_pnp.hip — PnPsolver (reference: src/PnPsolver.cc:67-950) for B problems (relocalisation candidates) as a chain of three
// launches on one stream:
//   k_pnp_ransac   one hypothesis per workgroup of one wave: EPnP on the 4 correspondences of its set, CheckInliers (:308-339)   sum of iterations
//   k_pnp_refine   one slot per workgroup of one wave: Refine (:260-305) on the flags of an iteration that is a record, or on    sum of iterations + B
//                  the prior best set; a slot that is no record returns at once
//   k_pnp_select   the replay of iterate's sequential loop (:165-258) over the counts and the refined counts                     B workgroups
// EPnP is double as in the reference; cvSVD of the symmetric MtM and PW0tPW0 is csrc/orbx_jacobi_eig.h (jacobi_eig<N>), cvInvert /
// cvSolve / cvSVD with CV_SVD are csrc/orbx_jacobi_svd.h's double flavour, qr_solve is restated literally.  DESIGN.md section 6
// ("k_pnp_*") has every expression tree; tests/pnp_ref.py is the same arithmetic in Python.  The model lives in LDS (PnpWork) and
// is formed ONCE per workgroup: sums over points are taken by one lane per output entry in ascending order, per-point values by
// the point's lane, the small serial solves by lane 0.  No floating-point value is combined across lanes: the inlier count is a
// ballot and a popcount, so the bytes do not depend on the launch shape.  Every loop has a bound that is a constant or an argument.
#ifdef ORBX_PNP_HOST
// tests/cpp/pnp_lockstep.cc compiles the kernels' text for the host as ONE thread per workgroup (tests/cpp/hip_lockstep.h comes
// first) and runs the workgroups one after the other.  Nothing below the kernels is compiled there.
#define PNP_T 1
#define PNP_BT 1
#else
#include "orbx_stage.h"
#define PNP_T 64      // k_pnp_ransac, k_pnp_refine: one wave
#define PNP_BT 256
#endif
#include <float.h>
#include <math.h>
#include "orbx_jacobi_eig.h"
#include "orbx_jacobi_svd.h"

// all arrays on the device; problem b owns correspondences off[b] .. off[b+1]-1, hypotheses soff[b] .. soff[b+1]-1 and refinement
// slots soff[b]+b .. soff[b+1]+b; its flags start at fbase[b] (= sum over the problems before it of iterations x n), its refined
// flags at rbase[b] (the same sum with iterations + 1); a slot's refinement points start at point rbase[b] + slot x n
struct PnpIn {
    const orbp_corr_t *corrs; const orbp_problem_t *prob; const int32_t *off, *soff, *sets, *hprob, *rprob; const int64_t *fbase, *rbase;
    const uint8_t *prior;
    int B, ncorr, nhyp;
};

// the model of one workgroup, in LDS
struct PnpWork {
    double cws[12], ccs[12], mtm[144], V[144], vv[48], l[60], rho[6], betas[4], Rs[27], ts[9], rep[3];
    double sum[16];           // the sums over points of the step at hand: 3 (centroid), 9 (PW0tPW0), 6 (pc0, pw0), 9 (ABt)
    double ci[9];             // cc_inv
    double W[66];             // the work array of the one-sided Jacobi, up to (6 + 5) x 5
    double sw[12], sb[6], sx[5];
    double ga[24], gb[6], gx[4], A1[4], A2[4];
    double U[9], Vr[9];
    int order[12];
    int neg;
};
#define PNP_PT 13             // doubles per point of a computation: pws 3, us 2, alphas 4, pcs 3, the reprojection term 1

__device__ __forceinline__ double pnp_dot(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ double pnp_dist2(const double *p1, const double *p2) {
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}
// entry (row 2 i + h, col) of M (fill_M, :436-451)
__device__ __forceinline__ double pnp_m(int h, int col, const double *as, double fu, double fv, double du, double dv) {
    const int k = col / 3, m = col % 3;
    if (m == 2) return as[k] * (h == 0 ? du : dv);
    if (m == h) return as[k] * (h == 0 ? fu : fv);
    return 0.0;
}

// qr_solve (:860-950) on the 6x4 A and b of gauss_newton; the early return on eta == 0 leaves x as it was
__device__ __forceinline__ void pnp_qr_solve(PnpWork &S) {
    const int nr = 6, nc = 4;
    double *pA = S.ga, *pb = S.gb, *pX = S.gx, *A1 = S.A1, *A2 = S.A2;
    for (int k = 0; k < nc; k++) {
        const int kk = k * nc + k;
        double eta = fabs(pA[kk]);
        for (int i = k + 1; i < nr; i++) {      // the reference's pointer advances AFTER the read: rows k .. nr-2 are looked at
            const double elt = fabs(pA[kk + (i - k - 1) * nc]);
            if (eta < elt) eta = elt;
        }
        if (eta == 0) { A1[k] = A2[k] = 0.0; return; }
        double sum = 0.0;
        const double inv_eta = 1. / eta;
        for (int i = k; i < nr; i++) {
            pA[i * nc + k] *= inv_eta;
            sum += pA[i * nc + k] * pA[i * nc + k];
        }
        double sigma = sqrt(sum);
        if (pA[kk] < 0) sigma = -sigma;
        pA[kk] += sigma;
        A1[k] = sigma * pA[kk];
        A2[k] = -eta * sigma;
        for (int j = k + 1; j < nc; j++) {
            double s2 = 0;
            for (int i = k; i < nr; i++) s2 += pA[i * nc + k] * pA[i * nc + j];
            const double tau = s2 / A1[k];
            for (int i = k; i < nr; i++) pA[i * nc + j] -= tau * pA[i * nc + k];
        }
    }
    for (int j = 0; j < nc; j++) {              // b <- Qt b
        double tau = 0;
        for (int i = j; i < nr; i++) tau += pA[i * nc + j] * pb[i];
        tau /= A1[j];
        for (int i = j; i < nr; i++) pb[i] -= tau * pA[i * nc + j];
    }
    pX[nc - 1] = pb[nc - 1] / A2[nc - 1];       // X = R-1 b
    for (int i = nc - 2; i >= 0; i--) {
        double sum = 0;
        for (int j = i + 1; j < nc; j++) sum += pA[i * nc + j] * pX[j];
        pX[i] = (pb[i] - sum) / A2[i];
    }
}

// find_betas_approx_1/2/3 (:667-758) and gauss_newton (:840-858): one thread
__device__ __forceinline__ void pnp_betas(PnpWork &S, int approx) {
    double *b = S.betas, *x = S.sx;
    const double *L = S.l;
    if (approx == 1) {
        const int cols[4] = {0, 1, 3, 6};
        for (int i = 0; i < 6; i++) for (int c = 0; c < 4; c++) S.W[i * 4 + c] = L[i * 10 + cols[c]];
        const double thr = jacobi_svd_d<6, 4>(S.W, S.sw);
        jacobi_backsub_d<6, 4>(S.W, S.sw, thr, S.rho, x);
        if (x[0] < 0) { b[0] = sqrt(-x[0]); b[1] = -x[1] / b[0]; b[2] = -x[2] / b[0]; b[3] = -x[3] / b[0]; }
        else { b[0] = sqrt(x[0]); b[1] = x[1] / b[0]; b[2] = x[2] / b[0]; b[3] = x[3] / b[0]; }
    } else if (approx == 2) {
        for (int i = 0; i < 6; i++) for (int c = 0; c < 3; c++) S.W[i * 3 + c] = L[i * 10 + c];
        const double thr = jacobi_svd_d<6, 3>(S.W, S.sw);
        jacobi_backsub_d<6, 3>(S.W, S.sw, thr, S.rho, x);
        if (x[0] < 0) { b[0] = sqrt(-x[0]); b[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0; }
        else { b[0] = sqrt(x[0]); b[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0; }
        if (x[1] < 0) b[0] = -b[0];
        b[2] = 0.0; b[3] = 0.0;
    } else {
        for (int i = 0; i < 6; i++) for (int c = 0; c < 5; c++) S.W[i * 5 + c] = L[i * 10 + c];
        const double thr = jacobi_svd_d<6, 5>(S.W, S.sw);
        jacobi_backsub_d<6, 5>(S.W, S.sw, thr, S.rho, x);
        if (x[0] < 0) { b[0] = sqrt(-x[0]); b[1] = (x[2] < 0) ? sqrt(-x[2]) : 0.0; }
        else { b[0] = sqrt(x[0]); b[1] = (x[2] > 0) ? sqrt(x[2]) : 0.0; }
        if (x[1] < 0) b[0] = -b[0];
        b[2] = x[3] / b[0];
        b[3] = 0.0;
    }
    for (int i = 0; i < 4; i++) S.gx[i] = 0.0;      // the reference leaves x uninitialised ("Not pinned")
    for (int k = 0; k < 5; k++) {
        for (int i = 0; i < 6; i++) {               // compute_A_and_b_gauss_newton (:812-838)
            const double *r = L + i * 10;
            double *a = S.ga + i * 4;
            a[0] = 2 * r[0] * b[0] + r[1] * b[1] + r[3] * b[2] + r[6] * b[3];
            a[1] = r[1] * b[0] + 2 * r[2] * b[1] + r[4] * b[2] + r[7] * b[3];
            a[2] = r[3] * b[0] + r[4] * b[1] + 2 * r[5] * b[2] + r[8] * b[3];
            a[3] = r[6] * b[0] + r[7] * b[1] + r[8] * b[2] + 2 * r[9] * b[3];
            S.gb[i] = S.rho[i] - (r[0] * b[0] * b[0] + r[1] * b[0] * b[1] + r[2] * b[1] * b[1] + r[3] * b[0] * b[2] + r[4] * b[1] * b[2] +
                                  r[5] * b[2] * b[2] + r[6] * b[0] * b[3] + r[7] * b[1] * b[3] + r[8] * b[2] * b[3] + r[9] * b[3] * b[3]);
        }
        pnp_qr_solve(S);
        for (int i = 0; i < 4; i++) b[i] += S.gx[i];
    }
}

// compute_pose (:477-525) on the np points whose pws and us are in pt (PNP_PT doubles per point: in LDS for a minimal set, in the
// thread's device scratch for a refinement), by the nth threads of one workgroup; R (9) and t (3) are left in S.Rs / S.ts at the
// returned approximation (1-3).  Entry and exit are barriers.
__device__ __forceinline__ int pnp_compute_pose(PnpWork &S, double *pt, int np, double fu, double fv, double uc, double vc, int tid, int nth) {
    const double dn = (double)np;
    __syncthreads();
    // choose_control_points (:375-409)
    for (int j = tid; j < 3; j += nth) {
        double s = 0;
        for (int i = 0; i < np; i++) s += pt[(size_t)i * PNP_PT + j];
        S.cws[j] = s / dn;
    }
    __syncthreads();
    for (int e = tid; e < 6; e += nth) {            // cvMulTransposed(PW0, PW0tPW0, 1): the upper triangle, rows ascending
        const int a = e < 3 ? 0 : (e < 5 ? 1 : 2), b = e < 3 ? e : (e < 5 ? e - 2 : 2);
        double s = 0.0;
        for (int i = 0; i < np; i++) s += (pt[(size_t)i * PNP_PT + a] - S.cws[a]) * (pt[(size_t)i * PNP_PT + b] - S.cws[b]);
        S.mtm[a * 3 + b] = s; S.mtm[b * 3 + a] = s;
    }
    __syncthreads();
    if (tid == 0) {
        jacobi_eig<3, false>(S.mtm, S.V, 0, 1);
        jacobi_eig_order<3>(S.mtm, S.sw, S.order);
        for (int i = 1; i < 4; i++) {
            const int o = S.order[i - 1];
            const double k = sqrt(S.sw[o] / dn);
            for (int j = 0; j < 3; j++) S.cws[i * 3 + j] = S.cws[j] + k * S.V[j * 3 + o];
        }
        // compute_barycentric_coordinates (:411-434): cvInvert(CC, CC_inv, CV_SVD)
        for (int i = 0; i < 3; i++)
            for (int j = 1; j < 4; j++) S.W[3 * i + j - 1] = S.cws[j * 3 + i] - S.cws[i];
        const double thr = jacobi_svd_d<3, 3>(S.W, S.sw);
        for (int c = 0; c < 3; c++) {
            for (int i = 0; i < 3; i++) S.sb[i] = (i == c) ? 1.0 : 0.0;
            jacobi_backsub_d<3, 3>(S.W, S.sw, thr, S.sb, S.sx);
            for (int k = 0; k < 3; k++) S.ci[k * 3 + c] = S.sx[k];
        }
    }
    __syncthreads();
    for (int i = tid; i < np; i += nth) {
        const double *pi = pt + (size_t)i * PNP_PT;
        double *a = pt + (size_t)i * PNP_PT + 5;
        for (int j = 0; j < 3; j++)
            a[1 + j] = S.ci[3 * j] * (pi[0] - S.cws[0]) + S.ci[3 * j + 1] * (pi[1] - S.cws[1]) + S.ci[3 * j + 2] * (pi[2] - S.cws[2]);
        a[0] = 1.0 - a[1] - a[2] - a[3];
    }
    __syncthreads();
    // cvMulTransposed(M, MtM, 1): the 78 entries of the upper triangle, each one lane's sum over the 2 np rows of M ascending
    for (int e = tid; e < 78; e += nth) {
        int r = 0, rem = e;
        for (int k = 0; k < 12; k++) if (rem >= 12 - r) { rem -= 12 - r; r++; }
        const int c = r + rem;
        double s = 0.0;
        for (int i = 0; i < np; i++) {
            const double *p = pt + (size_t)i * PNP_PT;
            const double du = uc - p[3], dv = vc - p[4];
            s += pnp_m(0, r, p + 5, fu, fv, du, dv) * pnp_m(0, c, p + 5, fu, fv, du, dv);
            s += pnp_m(1, r, p + 5, fu, fv, du, dv) * pnp_m(1, c, p + 5, fu, fv, du, dv);
        }
        S.mtm[r * 12 + c] = s; S.mtm[c * 12 + r] = s;
    }
    __syncthreads();
    jacobi_eig<12, PNP_T != 1>(S.mtm, S.V, tid, nth);
    __syncthreads();
    if (tid == 0) {
        jacobi_eig_order<12>(S.mtm, S.sw, S.order);
        for (int i = 0; i < 4; i++)                 // v[i] = ut + 12 * (11 - i)
            for (int k = 0; k < 12; k++) S.vv[i * 12 + k] = S.V[k * 12 + S.order[11 - i]];
        // compute_L_6x10 (:760-800), compute_rho (:802-810)
        for (int j = 0, a = 0, b = 1; j < 6; j++) {
            double dv[12];
            for (int i = 0; i < 4; i++)
                for (int k = 0; k < 3; k++) dv[i * 3 + k] = S.vv[i * 12 + 3 * a + k] - S.vv[i * 12 + 3 * b + k];
            double *row = S.l + 10 * j;
            row[0] = pnp_dot(dv, dv);
            row[1] = 2.0 * pnp_dot(dv, dv + 3);
            row[2] = pnp_dot(dv + 3, dv + 3);
            row[3] = 2.0 * pnp_dot(dv, dv + 6);
            row[4] = 2.0 * pnp_dot(dv + 3, dv + 6);
            row[5] = pnp_dot(dv + 6, dv + 6);
            row[6] = 2.0 * pnp_dot(dv, dv + 9);
            row[7] = 2.0 * pnp_dot(dv + 3, dv + 9);
            row[8] = 2.0 * pnp_dot(dv + 6, dv + 9);
            row[9] = pnp_dot(dv + 9, dv + 9);
            b++;
            if (b > 3) { a++; b = a + 1; }
        }
        S.rho[0] = pnp_dist2(S.cws, S.cws + 3); S.rho[1] = pnp_dist2(S.cws, S.cws + 6); S.rho[2] = pnp_dist2(S.cws, S.cws + 9);
        S.rho[3] = pnp_dist2(S.cws + 3, S.cws + 6); S.rho[4] = pnp_dist2(S.cws + 3, S.cws + 9); S.rho[5] = pnp_dist2(S.cws + 6, S.cws + 9);
    }
    for (int ap = 1; ap <= 3; ap++) {
        double *R = S.Rs + (ap - 1) * 9, *t = S.ts + (ap - 1) * 3;
        __syncthreads();
        if (tid == 0) {
            pnp_betas(S, ap);
            for (int k = 0; k < 12; k++) S.ccs[k] = 0.0;            // compute_ccs (:453-464)
            for (int i = 0; i < 4; i++)
                for (int k = 0; k < 12; k++) S.ccs[k] += S.betas[i] * S.vv[i * 12 + k];
        }
        __syncthreads();
        for (int i = tid; i < np; i += nth) {                       // compute_pcs (:466-475)
            const double *a = pt + (size_t)i * PNP_PT + 5;
            double *pc = pt + (size_t)i * PNP_PT + 9;
            for (int j = 0; j < 3; j++) pc[j] = a[0] * S.ccs[j] + a[1] * S.ccs[3 + j] + a[2] * S.ccs[6 + j] + a[3] * S.ccs[9 + j];
        }
        __syncthreads();
        if (tid == 0) S.neg = pt[9 + 2] < 0.0;                      // solve_for_sign (:636-649)
        __syncthreads();
        if (S.neg) {
            for (int k = tid; k < 12; k += nth) S.ccs[k] = -S.ccs[k];
            for (int i = tid; i < np; i += nth) {
                double *pc = pt + (size_t)i * PNP_PT + 9;
                pc[0] = -pc[0]; pc[1] = -pc[1]; pc[2] = -pc[2];
            }
        }
        __syncthreads();
        // estimate_R_and_t (:569-627)
        for (int e = tid; e < 6; e += nth) {
            const int o = e < 3 ? 9 + e : e - 3;
            double s = 0.0;
            for (int i = 0; i < np; i++) s += pt[(size_t)i * PNP_PT + o];
            S.sum[e] = s / dn;                                      // pc0 at 0..2, pw0 at 3..5
        }
        __syncthreads();
        for (int e = tid; e < 9; e += nth) {
            const int j = e / 3, c = e % 3;
            double s = 0.0;
            for (int i = 0; i < np; i++) s += (pt[(size_t)i * PNP_PT + 9 + j] - S.sum[j]) * (pt[(size_t)i * PNP_PT + c] - S.sum[3 + c]);
            S.sum[6 + e] = s;
        }
        __syncthreads();
        if (tid == 0) {
            svd3_d(S.sum + 6, S.W, S.U, S.Vr);
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) R[i * 3 + j] = pnp_dot(S.U + 3 * i, S.Vr + 3 * j);
            const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] - R[0] * R[5] * R[7];
            if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
            t[0] = S.sum[0] - pnp_dot(R, S.sum + 3);
            t[1] = S.sum[1] - pnp_dot(R + 3, S.sum + 3);
            t[2] = S.sum[2] - pnp_dot(R + 6, S.sum + 3);
        }
        __syncthreads();
        for (int i = tid; i < np; i += nth) {                       // reprojection_error (:550-567): the terms
            double *p = pt + (size_t)i * PNP_PT;
            const double Xc = pnp_dot(R, p) + t[0], Yc = pnp_dot(R + 3, p) + t[1];
            const double inv_Zc = 1.0 / (pnp_dot(R + 6, p) + t[2]);
            const double ue = uc + fu * Xc * inv_Zc, ve = vc + fv * Yc * inv_Zc;
            const double u = p[3], v = p[4];
            p[12] = sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
        }
        __syncthreads();
        if (tid == 0) {
            double sum2 = 0.0;
            for (int i = 0; i < np; i++) sum2 += pt[(size_t)i * PNP_PT + 12];
            S.rep[ap - 1] = sum2 / dn;
        }
    }
    __syncthreads();
    int N = 1;
    if (S.rep[1] < S.rep[0]) N = 2;
    if (S.rep[2] < S.rep[N - 1]) N = 3;
    return N;
}

// CheckInliers (:308-339) over the n correspondences of a problem: correspondence i belongs to lane i % nth
__device__ __forceinline__ int pnp_check_inliers(const orbp_corr_t *cr, int n, const double *R, const double *t, double fu, double fv,
                                                 double uc, double vc, float th2, uint8_t *fl, int tid, int nth) {
    int cnt = 0;
    for (int base = 0; base < n; base += nth) {
        const int i = base + tid;
        bool inl = false;
        if (i < n) {
            const orbp_corr_t c = cr[i];
            const double x = (double)c.w[0], y = (double)c.w[1], z = (double)c.w[2];
            const float Xc = (float)(R[0] * x + R[1] * y + R[2] * z + t[0]);
            const float Yc = (float)(R[3] * x + R[4] * y + R[5] * z + t[1]);
            const float invZc = (float)(1 / (R[6] * x + R[7] * y + R[8] * z + t[2]));
            const double ue = uc + fu * (double)Xc * (double)invZc;
            const double ve = vc + fv * (double)Yc * (double)invZc;
            const float distX = (float)((double)c.u - ue), distY = (float)((double)c.v - ve);
            const float error2 = distX * distX + distY * distY;
            inl = error2 < c.sigma2 * th2;       // a NaN compares false
            fl[i] = inl ? 1 : 0;
        }
        cnt += __popcll(__ballot(inl));
    }
    return cnt;
}

__device__ __forceinline__ void pnp_store_model(const double *R, const double *t, double *m, float *T) {
    for (int k = 0; k < 9; k++) m[k] = R[k];
    for (int k = 0; k < 3; k++) m[9 + k] = t[k];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[i * 4 + j] = (float)R[i * 3 + j];
        T[i * 4 + 3] = (float)t[i];
    }
    T[12] = 0.f; T[13] = 0.f; T[14] = 0.f; T[15] = 1.f;
}

// ---- one hypothesis per workgroup
__global__ __launch_bounds__(PNP_T) void k_pnp_ransac(PnpIn in, double *__restrict__ models, float *__restrict__ tcws, int32_t *__restrict__ choices,
                                                      int32_t *__restrict__ counts, uint8_t *__restrict__ flags) {
    __shared__ PnpWork S;
    __shared__ double pt[4 * PNP_PT];
    const int tid = threadIdx.x, hyp = blockIdx.x, b = in.hprob[hyp];
    const int first = in.off[b], n = in.off[b + 1] - first, it = hyp - in.soff[b];
    const orbp_problem_t pb = in.prob[b];
    const orbp_corr_t *cr = in.corrs + first;
    const double fu = (double)pb.K[0], fv = (double)pb.K[1], uc = (double)pb.K[2], vc = (double)pb.K[3];
    for (int i = tid; i < 4; i += PNP_T) {       // add_correspondence (:363-373)
        const orbp_corr_t c = cr[in.sets[(size_t)hyp * 4 + i]];
        double *p = pt + i * PNP_PT;
        p[0] = (double)c.w[0]; p[1] = (double)c.w[1]; p[2] = (double)c.w[2]; p[3] = (double)c.u; p[4] = (double)c.v;
    }
    const int N = pnp_compute_pose(S, pt, 4, fu, fv, uc, vc, tid, PNP_T);
    const double *R = S.Rs + (N - 1) * 9, *t = S.ts + (N - 1) * 3;
    if (tid == 0) {
        pnp_store_model(R, t, models + (size_t)hyp * 12, tcws + (size_t)hyp * 16);
        choices[hyp] = N;
    }
    const int cnt = pnp_check_inliers(cr, n, R, t, fu, fv, uc, vc, pb.th2, flags + in.fbase[b] + (int64_t)it * n, tid, PNP_T);
    if (tid == 0) counts[hyp] = cnt;
}

// ---- Refine (:260-305): one slot per workgroup; slot i < iterations refines iteration i's flags, slot `iterations` the prior best set
__global__ __launch_bounds__(PNP_T) void k_pnp_refine(PnpIn in, const int32_t *__restrict__ counts, const uint8_t *__restrict__ flags,
                                                      double *__restrict__ points, double *__restrict__ rmodels, float *__restrict__ rtcws,
                                                      int32_t *__restrict__ rcounts, uint8_t *__restrict__ rflags) {
    __shared__ PnpWork S;
    const int tid = threadIdx.x, gs = blockIdx.x, b = in.rprob[gs];
    const int first = in.off[b], n = in.off[b + 1] - first, h0 = in.soff[b], its = in.soff[b + 1] - h0, slot = gs - (h0 + b);
    const orbp_problem_t pb = in.prob[b];
    uint8_t *rfl = rflags + in.rbase[b] + (int64_t)slot * n;
    // a record: a strict prefix maximum of the counts that is >= min_inliers and above the prior best count; the prior slot: a non-empty set
    bool record;
    if (slot == its) record = pb.prior_best_inliers > 0 && its > 0 && n >= pb.min_inliers;
    else {
        const int c = counts[h0 + slot];
        record = c >= pb.min_inliers && c > pb.prior_best_inliers;
        for (int k = 0; k < slot; k++) if (counts[h0 + k] >= c) record = false;
    }
    if (!record) {
        if (tid == 0) {
            rcounts[gs] = -1;
            for (int k = 0; k < 12; k++) rmodels[(size_t)gs * 12 + k] = 0.0;
            for (int k = 0; k < 16; k++) rtcws[(size_t)gs * 16 + k] = 0.f;
        }
        for (int i = tid; i < n; i += PNP_T) rfl[i] = 0;
        return;
    }
    const orbp_corr_t *cr = in.corrs + first;
    const uint8_t *src = slot == its ? in.prior + first : flags + in.fbase[b] + (int64_t)slot * n;
    double *pt = points + ((size_t)(in.rbase[b] + (int64_t)slot * n)) * PNP_PT;
    int np = 0;
    for (int base = 0; base < n; base += PNP_T) {           // the flagged correspondences in ascending index
        const int i = base + tid;
        const bool f = i < n && src[i] != 0;
        const unsigned long long m = __ballot(f);
        if (f) {
            const orbp_corr_t c = cr[i];
            double *p = pt + (size_t)(np + __popcll(m & ((1ull << tid) - 1ull))) * PNP_PT;
            p[0] = (double)c.w[0]; p[1] = (double)c.w[1]; p[2] = (double)c.w[2]; p[3] = (double)c.u; p[4] = (double)c.v;
        }
        np += __popcll(m);
    }
    const double fu = (double)pb.K[0], fv = (double)pb.K[1], uc = (double)pb.K[2], vc = (double)pb.K[3];
    const int N = pnp_compute_pose(S, pt, np, fu, fv, uc, vc, tid, PNP_T);
    const double *R = S.Rs + (N - 1) * 9, *t = S.ts + (N - 1) * 3;
    if (tid == 0) pnp_store_model(R, t, rmodels + (size_t)gs * 12, rtcws + (size_t)gs * 16);
    const int cnt = pnp_check_inliers(cr, n, R, t, fu, fv, uc, vc, pb.th2, rfl, tid, PNP_T);
    if (tid == 0) rcounts[gs] = cnt;
}

// ---- iterate's loop (:165-258) over the counts and refined counts of one problem per workgroup
__global__ __launch_bounds__(PNP_BT) void k_pnp_select(PnpIn in, const float *__restrict__ tcws, const int32_t *__restrict__ counts,
                                                     const uint8_t *__restrict__ flags, const float *__restrict__ rtcws,
                                                     const int32_t *__restrict__ rcounts, const uint8_t *__restrict__ rflags,
                                                     uint8_t *__restrict__ retInl, uint8_t *__restrict__ bestOut, orbp_pnp_info_t *__restrict__ infos) {
    __shared__ int s_ret, s_best;       // which flags to return / to keep: -2 none, -1 the prior set, i >= 0 iteration i's (s_ret: the refined ones of slot i, `its` = the prior slot, when s_hit)
    __shared__ int s_hit;
    const int tid = threadIdx.x, b = blockIdx.x;
    const int first = in.off[b], n = in.off[b + 1] - first, h0 = in.soff[b], its = in.soff[b + 1] - h0, r0 = h0 + b;
    if (tid == 0) {
        const orbp_problem_t pb = in.prob[b];
        const int minInl = pb.min_inliers;
        orbp_pnp_info_t o;
        o.n = n; o.iterations = its; o.hit_iteration = -1; o.iterations_run = 0; o.best_iteration = -1; o.best_inliers = pb.prior_best_inliers;
        o.refined_inliers = 0; o.no_more = 0; o.pose = ORBP_POSE_NONE;
        for (int k = 0; k < 16; k++) { o.Tcw[k] = 0.f; o.best_Tcw[k] = 0.f; }
        int ret = -2, hit = 0;
        if (n < minInl || its == 0) o.no_more = 1;              // :173-177
        else {
            int best = pb.prior_best_inliers, bestIt = -1;
            for (int it = 0; it < its; it++) {
                o.iterations_run++;
                const int c = counts[h0 + it];
                if (c >= minInl) {
                    if (c > best) { best = c; bestIt = it; }
                    const int slot = bestIt < 0 ? its : bestIt;
                    const int rc = rcounts[r0 + slot];
                    if (rc > minInl) {
                        o.hit_iteration = it; o.refined_inliers = rc; o.pose = ORBP_POSE_REFINED;
                        for (int k = 0; k < 16; k++) o.Tcw[k] = rtcws[(size_t)(r0 + slot) * 16 + k];
                        ret = slot; hit = 1;
                        break;
                    }
                }
            }
            o.best_iteration = bestIt; o.best_inliers = best;
            if (bestIt >= 0) for (int k = 0; k < 16; k++) o.best_Tcw[k] = tcws[(size_t)(h0 + bestIt) * 16 + k];
            if (!hit && pb.iterations_done + o.iterations_run >= pb.max_iterations) {   // :241-255
                o.no_more = 1;
                if (best >= minInl) {
                    o.pose = bestIt >= 0 ? ORBP_POSE_BEST : ORBP_POSE_PRIOR_BEST;
                    for (int k = 0; k < 16; k++) o.Tcw[k] = o.best_Tcw[k];
                    ret = bestIt;
                }
            }
        }
        s_ret = ret; s_hit = hit; s_best = o.best_iteration >= 0 ? o.best_iteration : (pb.prior_best_inliers > 0 ? -1 : -2);
        infos[b] = o;
    }
    __syncthreads();
    const int ret = s_ret, hit = s_hit, best = s_best;
    const uint8_t *pr = in.prior + first, *fl = flags + in.fbase[b], *rf = rflags + in.rbase[b];
    for (int i = tid; i < n; i += PNP_BT) {
        retInl[first + i] = ret == -2 ? 0 : (hit ? rf[(int64_t)ret * n + i] : (ret == -1 ? pr[i] : fl[(int64_t)ret * n + i]));
        bestOut[first + i] = best == -2 ? 0 : (best == -1 ? pr[i] : fl[(int64_t)best * n + i]);
    }
}

#ifndef ORBX_PNP_HOST
// ------------------------------------------------------------------------------------
// host side: this thread's staging pair (orbx_stage.h)
static thread_local StagePair g_ps;
void orbx_internal_release_pnp_scratch() { g_ps.release(); }
#define PNP_MAX_TOTAL (1 << 24)     // correspondences, and hypotheses, of one call

extern "C" int orbp_pnp_parameters(int n, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                                   int *adj_min_inliers, int *adj_max_iterations) {
    if (!adj_min_inliers || !adj_max_iterations || n < 0) { orbx_set_error("orbp_pnp_parameters: bad arguments"); return ORBX_ERR_ARG; }
    if (min_set != 4) { orbx_set_error("orbp_pnp_parameters: min_set = %d; EPnP here takes 4", min_set); return ORBX_ERR_ARG; }
    int nMinInliers = (int)((float)n * epsilon);        // int nMinInliers = N*mRansacEpsilon
    if (nMinInliers < min_inliers) nMinInliers = min_inliers;
    if (nMinInliers < min_set) nMinInliers = min_set;
    if (epsilon < (float)nMinInliers / n) epsilon = (float)nMinInliers / n;
    int nIterations;
    if (nMinInliers == n)
        nIterations = 1;
    else {   // ceil(...) converts a double to int: kept in range here, where the reference's conversion is undefined
        const double k = ceil(log(1 - probability) / log(1 - pow(epsilon, 3)));
        nIterations = !(k < (double)max_iterations) ? max_iterations : (k < 1.0 ? 1 : (int)k);
    }
    *adj_min_inliers = nMinInliers;
    *adj_max_iterations = std::max(1, std::min(nIterations, max_iterations));
    return ORBX_OK;
}

extern "C" int orbp_pnp_ransac_batch(const orbp_corr_t *corrs, const int32_t *offsets, int B, const orbp_problem_t *problems,
                                     const int32_t *sets, const int32_t *set_offsets, const uint8_t *prior_best_flags, int32_t *counts,
                                     double *models, float *tcws, int32_t *choices, uint8_t *flags, int32_t *refined_counts,
                                     uint8_t *inliers, uint8_t *best_flags, orbp_pnp_info_t *infos, int device) {
    const char *fn = "orbp_pnp_ransac_batch";
    if (!corrs || !offsets || !problems || !sets || !set_offsets || !counts || !inliers || !best_flags || !infos || B < 0) {
        orbx_set_error("%s: bad arguments", fn); return ORBX_ERR_ARG;
    }
    if (B == 0) return ORBX_OK;
    if (offsets[0] < 0 || set_offsets[0] < 0) { orbx_set_error("%s: negative offset", fn); return ORBX_ERR_ARG; }
    size_t nflags = 0, nrflags = 0;
    for (int b = 0; b < B; b++) {
        const int n = offsets[b + 1] - offsets[b], its = set_offsets[b + 1] - set_offsets[b];
        if (offsets[b + 1] < offsets[b] || set_offsets[b + 1] < set_offsets[b]) { orbx_set_error("%s: offsets decrease at problem %d", fn, b); return ORBX_ERR_ARG; }
        if (offsets[b + 1] > PNP_MAX_TOTAL || set_offsets[b + 1] > PNP_MAX_TOTAL) { orbx_set_error("%s: more than %d correspondences or sets", fn, PNP_MAX_TOTAL); return ORBX_ERR_ARG; }
        if (its > 0 && n < 4) { orbx_set_error("%s: problem %d has %d correspondences, 4 are needed", fn, b, n); return ORBX_ERR_ARG; }
        if (its > 0 && n < problems[b].min_inliers) { orbx_set_error("%s: problem %d has sets but fewer correspondences (%d) than min_inliers", fn, b, n); return ORBX_ERR_ARG; }
        if (problems[b].prior_best_inliers < 0 || problems[b].iterations_done < 0) { orbx_set_error("%s: problem %d has a negative prior state", fn, b); return ORBX_ERR_ARG; }
        int prior = 0;
        for (int i = offsets[b]; i < offsets[b + 1]; i++) {
            const float s2 = corrs[i].sigma2;
            if (!(s2 >= 0.f) || !std::isfinite(s2)) {
                orbx_set_error("%s: correspondence %d of problem %d has a sigma2 that is negative or not finite", fn, i - offsets[b], b); return ORBX_ERR_ARG;
            }
            if (prior_best_flags && prior_best_flags[i]) prior++;
        }
        if (prior != problems[b].prior_best_inliers) {
            orbx_set_error("%s: problem %d: prior count %d, %d prior flags set", fn, b, problems[b].prior_best_inliers, prior); return ORBX_ERR_ARG;
        }
        for (int h = set_offsets[b]; h < set_offsets[b + 1]; h++) {
            const int32_t *s = sets + (size_t)h * 4;
            for (int k = 0; k < 4; k++) {
                if (s[k] < 0 || s[k] >= n) { orbx_set_error("%s: set %d of problem %d names a correspondence out of %d", fn, h - set_offsets[b], b, n); return ORBX_ERR_ARG; }
                for (int j = 0; j < k; j++)
                    if (s[j] == s[k]) { orbx_set_error("%s: set %d of problem %d names a correspondence twice", fn, h - set_offsets[b], b); return ORBX_ERR_ARG; }
            }
        }
        nflags += (size_t)its * n;
        nrflags += ((size_t)its + 1) * n;
    }
    if (nrflags > ((size_t)1 << 24)) { orbx_set_error("%s: %zu refinement points", fn, nrflags); return ORBX_ERR_ARG; }
    const int p0 = offsets[0], h0 = set_offsets[0], np = offsets[B] - p0, nh = set_offsets[B] - h0, ns = nh + B;
    StagePlan pl;
    // upload block: corrs | problems | off | soff | sets | hprob | rprob | fbase | rbase | prior;  download block: infos | counts |
    // choices | rcounts | inliers | best | models | tcws | flags;  device only: refined models, poses and flags, the refinement points
    const size_t oCo = pl.take((size_t)np * sizeof(orbp_corr_t)), oPr = pl.take((size_t)B * sizeof(orbp_problem_t));
    const size_t oOf = pl.take(((size_t)B + 1) * 4), oSo = pl.take(((size_t)B + 1) * 4), oSe = pl.take((size_t)nh * 16);
    const size_t oHp = pl.take((size_t)nh * 4), oRp = pl.take((size_t)ns * 4), oFb = pl.take((size_t)B * 8), oRb = pl.take((size_t)B * 8);
    const size_t oPi = pl.take((size_t)np);
    pl.mark_inputs();
    const size_t oInfo = pl.take((size_t)B * sizeof(orbp_pnp_info_t)), oCnt = pl.take((size_t)nh * 4), oCh = pl.take((size_t)nh * 4);
    const size_t oRc = pl.take((size_t)ns * 4), oInl = pl.take((size_t)np), oBest = pl.take((size_t)np);
    const size_t oMod = pl.take((size_t)nh * 96), oTc = pl.take((size_t)nh * 64), oFl = pl.take(nflags), oDnEnd = pl.off;
    const size_t oRm = pl.take((size_t)ns * 96), oRt = pl.take((size_t)ns * 64), oRf = pl.take(nrflags);
    const size_t oPt = pl.take(nrflags * PNP_PT * 8);
    int rc = g_ps.reserve(device, pl.off, (size_t)1 << 20);
    if (rc) return rc;
    uint8_t *d = g_ps.d, *h = g_ps.h;
    const hipStream_t st = g_ps.stream;
    memcpy(h + oCo, corrs + p0, (size_t)np * sizeof(orbp_corr_t));
    memcpy(h + oPr, problems, (size_t)B * sizeof(orbp_problem_t));
    memcpy(h + oSe, sets + (size_t)h0 * 4, (size_t)nh * 16);
    if (prior_best_flags) memcpy(h + oPi, prior_best_flags + p0, (size_t)np); else memset(h + oPi, 0, (size_t)np);
    int32_t *hOf = (int32_t *)(h + oOf), *hSo = (int32_t *)(h + oSo), *hHp = (int32_t *)(h + oHp), *hRp = (int32_t *)(h + oRp);
    int64_t *hFb = (int64_t *)(h + oFb), *hRb = (int64_t *)(h + oRb);
    int64_t fb = 0, rb = 0;
    for (int b = 0; b < B; b++) {
        const int n = offsets[b + 1] - offsets[b], its = set_offsets[b + 1] - set_offsets[b], s0 = set_offsets[b] - h0;
        hOf[b] = offsets[b] - p0; hSo[b] = s0; hFb[b] = fb; hRb[b] = rb;
        for (int k = 0; k < its; k++) hHp[s0 + k] = b;
        for (int k = 0; k <= its; k++) hRp[s0 + b + k] = b;
        fb += (int64_t)its * n; rb += (int64_t)(its + 1) * n;
    }
    hOf[B] = np; hSo[B] = nh;
    ORBX_HIP(hipMemcpyAsync(d, h, pl.in_end, hipMemcpyHostToDevice, st));
    PnpIn in;
    in.corrs = (const orbp_corr_t *)(d + oCo); in.prob = (const orbp_problem_t *)(d + oPr); in.off = (const int32_t *)(d + oOf);
    in.soff = (const int32_t *)(d + oSo); in.sets = (const int32_t *)(d + oSe); in.hprob = (const int32_t *)(d + oHp);
    in.rprob = (const int32_t *)(d + oRp); in.fbase = (const int64_t *)(d + oFb); in.rbase = (const int64_t *)(d + oRb);
    in.prior = d + oPi; in.B = B; in.ncorr = np; in.nhyp = nh;
    int32_t *dcnt = (int32_t *)(d + oCnt), *drc = (int32_t *)(d + oRc);
    (void)hipGetLastError();
    if (nh > 0) {
        hipLaunchKernelGGL(k_pnp_ransac, dim3((unsigned)nh), dim3(PNP_T), 0, st, in, (double *)(d + oMod), (float *)(d + oTc), (int32_t *)(d + oCh), dcnt, d + oFl);
        hipLaunchKernelGGL(k_pnp_refine, dim3((unsigned)ns), dim3(PNP_T), 0, st, in, (const int32_t *)dcnt, (const uint8_t *)(d + oFl), (double *)(d + oPt),
                           (double *)(d + oRm), (float *)(d + oRt), drc, d + oRf);
    }
    hipLaunchKernelGGL(k_pnp_select, dim3((unsigned)B), dim3(PNP_BT), 0, st, in, (const float *)(d + oTc), (const int32_t *)dcnt, (const uint8_t *)(d + oFl),
                       (const float *)(d + oRt), (const int32_t *)drc, (const uint8_t *)(d + oRf), d + oInl, d + oBest, (orbp_pnp_info_t *)(d + oInfo));
    ORBX_HIP(hipGetLastError());
    const size_t dnEnd = flags ? oDnEnd : ((models || tcws) ? oFl : oMod);
    ORBX_HIP(hipMemcpyAsync(h + oInfo, d + oInfo, dnEnd - oInfo, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    memcpy(infos, h + oInfo, (size_t)B * sizeof(orbp_pnp_info_t));
    memcpy(inliers + p0, h + oInl, (size_t)np);
    memcpy(best_flags + p0, h + oBest, (size_t)np);
    if (nh > 0) {
        memcpy(counts + h0, h + oCnt, (size_t)nh * 4);
        if (choices) memcpy(choices + h0, h + oCh, (size_t)nh * 4);
        if (refined_counts) memcpy(refined_counts + h0, h + oRc, (size_t)ns * 4);
        if (models) memcpy(models + (size_t)h0 * 12, h + oMod, (size_t)nh * 96);
        if (tcws) memcpy(tcws + (size_t)h0 * 16, h + oTc, (size_t)nh * 64);
        if (flags) memcpy(flags, h + oFl, nflags);
    } else if (refined_counts) {
        for (int k = 0; k < ns; k++) refined_counts[h0 + k] = -1;
    }
    return ORBX_OK;
}

extern "C" int orbp_pnp_ransac(const orbp_corr_t *corrs, int n, const orbp_problem_t *problem, const int32_t *sets, int iterations,
                               const uint8_t *prior_best_flags, int32_t *counts, double *models, float *tcws, int32_t *choices,
                               uint8_t *flags, int32_t *refined_counts, uint8_t *inliers, uint8_t *best_flags, orbp_pnp_info_t *info, int device) {
    if (n < 0 || iterations < 0) { orbx_set_error("orbp_pnp_ransac: n = %d, iterations = %d", n, iterations); return ORBX_ERR_ARG; }
    const int32_t off[2] = {0, n}, soff[2] = {0, iterations};
    return orbp_pnp_ransac_batch(corrs, off, 1, problem, sets, soff, prior_best_flags, counts, models, tcws, choices, flags, refined_counts,
                                 inliers, best_flags, info, device);
}
#endif   // ORBX_PNP_HOST
