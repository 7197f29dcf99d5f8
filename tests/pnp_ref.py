"""PnPsolver (src/PnPsolver.cc) restated in Python, operation for operation as csrc/orbx_pnp.hip does it (DESIGN.md section 6,
"k_pnp_*").  EPnP is double: Python floats ARE IEEE doubles and math.sqrt is the correctly rounded square root, so the small
solves are written out scalar by scalar, in the kernel's order; sums over points are left-to-right (numpy's cumulative sum is a
sequential loop, seqsum), per-point values and CheckInliers are numpy vectors with explicit float32 narrowing.  The five OpenCV
calls are this library's own: jacobi_eig (csrc/orbx_jacobi_eig.h) and the double one-sided Jacobi (csrc/orbx_jacobi_svd.h)."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
CORR_DTYPE = np.dtype([("w", "<f4", (3,)), ("u", "<f4"), ("v", "<f4"), ("sigma2", "<f4")])
PROBLEM_DTYPE = np.dtype([("K", "<f4", (4,)), ("th2", "<f4"), ("min_inliers", "<i4"), ("max_iterations", "<i4"),
                          ("iterations_done", "<i4"), ("prior_best_inliers", "<i4")])
INFO_DTYPE = np.dtype([("n", "<i4"), ("iterations", "<i4"), ("hit_iteration", "<i4"), ("iterations_run", "<i4"), ("best_iteration", "<i4"),
                       ("best_inliers", "<i4"), ("refined_inliers", "<i4"), ("no_more", "<i4"), ("pose", "<i4"),
                       ("Tcw", "<f4", (16,)), ("best_Tcw", "<f4", (16,))])
POSE_NONE, POSE_REFINED, POSE_BEST, POSE_PRIOR_BEST = 0, 1, 2, 3
MAX_SWEEPS = 30
DBL_EPS = float(np.finfo(np.float64).eps)
NAN = float("nan")


def sqrt(x):
    return math.sqrt(x) if x >= 0 else (NAN if x == x else x)      # sqrt(negative) = NaN, sqrt(NaN) = NaN, no exception


def div(a, b):
    """IEEE double division, x / 0 included"""
    if b != 0:
        return a / b
    if a != a or a == 0:
        return NAN
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def seqsum(a):
    """0.0 + a[0] + a[1] + .. left to right, along axis 0"""
    a = np.asarray(a, f64)
    with np.errstate(all="ignore"):
        return np.cumsum(np.concatenate([np.zeros((1,) + a.shape[1:]), a], axis=0), axis=0)[-1]


def jacobi_eig(A):
    """csrc/orbx_jacobi_eig.h, jacobi_eig<N>: A [N][N] list of lists (symmetric) -> (A rotated, V with the eigenvectors in columns)"""
    N = len(A)
    A = [list(map(float, r)) for r in A]
    V = [[1.0 if i == j else 0.0 for j in range(N)] for i in range(N)]
    ss = 0.0
    for i in range(N):
        for j in range(N):
            ss += A[i][j] * A[i][j]
    thr = DBL_EPS * sqrt(ss)
    for _ in range(MAX_SWEEPS):
        changed = False
        for p in range(N - 1):
            for q in range(p + 1, N):
                g, app, aqq = A[p][q], A[p][p], A[q][q]
                if not abs(g) > thr:
                    continue
                changed = True
                theta = div(aqq - app, 2.0 * g)
                t = div(1.0, abs(theta) + sqrt(theta * theta + 1.0))
                if theta < 0.0:
                    t = -t
                c = div(1.0, sqrt(t * t + 1.0))
                s = t * c
                A[p][p] = app - t * g; A[p][q] = 0.0
                A[q][q] = aqq + t * g; A[q][p] = 0.0
                for k in range(N):
                    if k == p or k == q:
                        continue
                    x, y = A[k][p], A[k][q]
                    A[k][p] = A[p][k] = c * x - s * y
                    A[k][q] = A[q][k] = s * x + c * y
                for r in range(N):
                    x, y = V[r][p], V[r][q]
                    V[r][p] = c * x - s * y
                    V[r][q] = s * x + c * y
        if not changed:
            break
    return A, V


def stable_order(w):
    """the columns by descending w, of equal values the lower first; a NaN compares false and stays where it is"""
    used, order = set(), []
    for _ in range(len(w)):
        best = -1
        for j in range(len(w)):
            if j not in used and (best < 0 or w[j] > w[best]):
                best = j
        used.add(best)
        order.append(best)
    return order


def eig_sym(A):
    """cvSVD(A, D, Ut, 0, MODIFY_A | U_T) of a symmetric positive semi-definite A as the kernel takes it -> (d [N] descending, ut [N][N])"""
    N = len(A)
    Ar, V = jacobi_eig(A)
    w = [abs(Ar[j][j]) for j in range(N)]
    order = stable_order(w)
    return [w[o] for o in order], [[V[r][o] for r in range(N)] for o in order]


def jacobi_sweeps_d(W, M, N):
    for _ in range(MAX_SWEEPS):
        changed = False
        for p in range(N - 1):
            for q in range(p + 1, N):
                a = b = g = 0.0
                for i in range(M):
                    x, y = W[i][p], W[i][q]
                    a += x * x; b += y * y; g += x * y
                if not abs(g) > (2.0 * DBL_EPS) * sqrt(a * b):
                    continue
                changed = True
                g2, beta = 2.0 * g, a - b
                gamma = sqrt(g2 * g2 + beta * beta)
                if beta < 0.0:
                    s = sqrt(div((gamma - beta) * 0.5, gamma))
                    c = div(g2, (gamma * s) * 2.0)
                else:
                    c = sqrt(div(gamma + beta, gamma * 2.0))
                    s = div(g2, (gamma * c) * 2.0)
                for r in range(M + N):
                    x, y = W[r][p], W[r][q]
                    W[r][p] = c * x + s * y
                    W[r][q] = c * y - s * x
        if not changed:
            break


def jacobi_svd_d(A):
    """A [M][N] -> (W [M + N][N], w [N], thr)"""
    M, N = len(A), len(A[0])
    W = [list(map(float, r)) for r in A] + [[1.0 if i == j else 0.0 for j in range(N)] for i in range(N)]
    jacobi_sweeps_d(W, M, N)
    w, total = [], 0.0
    for j in range(N):
        a = 0.0
        for i in range(M):
            a += W[i][j] * W[i][j]
        w.append(sqrt(a))
        total += w[j]
    return W, w, (2.0 * DBL_EPS) * total


def backsub_d(W, w, thr, b):
    N, M = len(w), len(W) - len(w)
    x = [0.0] * N
    for j in range(N):
        if not w[j] > thr:
            continue
        s = 0.0
        for i in range(M):
            s += W[i][j] * b[i]
        coef = div(div(s, w[j]), w[j])
        for k in range(N):
            x[k] += W[M + k][j] * coef
    return x


def svd_solve(A, b):
    """cvSolve(A, b, x, CV_SVD)"""
    W, w, thr = jacobi_svd_d(A)
    return backsub_d(W, w, thr, b)


def svd_invert3(A):
    """cvInvert(A, inv, CV_SVD) of a 3x3"""
    W, w, thr = jacobi_svd_d(A)
    inv = [[0.0] * 3 for _ in range(3)]
    for c in range(3):
        x = backsub_d(W, w, thr, [1.0 if i == c else 0.0 for i in range(3)])
        for k in range(3):
            inv[k][c] = x[k]
    return inv


def svd3_d(A):
    """cvSVD(A, D, U, V, MODIFY_A) of a 3x3 -> (U [3][3], V [3][3] not transposed, w descending)"""
    W = [list(map(float, r)) for r in A] + [[1.0 if i == j else 0.0 for j in range(3)] for i in range(3)]
    jacobi_sweeps_d(W, 3, 3)
    w = []
    for j in range(3):
        a = 0.0
        for i in range(3):
            a += W[i][j] * W[i][j]
        w.append(sqrt(a))
    o = stable_order(w)
    U = [[0.0] * 3 for _ in range(3)]
    V = [[W[3 + i][o[k]] for k in range(3)] for i in range(3)]
    for i in range(3):
        U[i][0] = div(W[i][o[0]], w[o[0]])
        U[i][1] = div(W[i][o[1]], w[o[1]])
    u2 = [U[1][0] * U[2][1] - U[2][0] * U[1][1], U[2][0] * U[0][1] - U[0][0] * U[2][1], U[0][0] * U[1][1] - U[1][0] * U[0][1]]
    d = 0.0
    for i in range(3):
        d += u2[i] * W[i][o[2]]
    for i in range(3):
        U[i][2] = -u2[i] if d < 0.0 else u2[i]
    return U, V, [w[k] for k in o]


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def dist2(p1, p2):
    return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2])


def qr_solve(A, b, x):
    """:860-950 on the 6x4 A (flat list of 24), b (6), x (4): all modified in place; the early return leaves x as it was"""
    nr, nc = 6, 4
    A1, A2 = [0.0] * nc, [0.0] * nc
    for k in range(nc):
        kk = k * nc + k
        eta = abs(A[kk])
        for i in range(k + 1, nr):
            elt = abs(A[kk + (i - k - 1) * nc])
            if eta < elt:
                eta = elt
        if eta == 0:
            return
        s, inv_eta = 0.0, div(1.0, eta)
        for i in range(k, nr):
            A[i * nc + k] *= inv_eta
            s += A[i * nc + k] * A[i * nc + k]
        sigma = sqrt(s)
        if A[kk] < 0:
            sigma = -sigma
        A[kk] += sigma
        A1[k] = sigma * A[kk]
        A2[k] = -eta * sigma
        for j in range(k + 1, nc):
            s2 = 0.0
            for i in range(k, nr):
                s2 += A[i * nc + k] * A[i * nc + j]
            tau = div(s2, A1[k])
            for i in range(k, nr):
                A[i * nc + j] -= tau * A[i * nc + k]
    for j in range(nc):
        tau = 0.0
        for i in range(j, nr):
            tau += A[i * nc + j] * b[i]
        tau = div(tau, A1[j])
        for i in range(j, nr):
            b[i] -= tau * A[i * nc + j]
    x[nc - 1] = div(b[nc - 1], A2[nc - 1])
    for i in range(nc - 2, -1, -1):
        s = 0.0
        for j in range(i + 1, nc):
            s += A[i * nc + j] * x[j]
        x[i] = div(b[i] - s, A2[i])


def find_betas(L, rho, approx):
    cols = {1: (0, 1, 3, 6), 2: (0, 1, 2), 3: (0, 1, 2, 3, 4)}[approx]
    x = svd_solve([[L[i][c] for c in cols] for i in range(6)], rho)
    b = [0.0] * 4
    if approx == 1:
        if x[0] < 0:
            b[0] = sqrt(-x[0]); b[1] = div(-x[1], b[0]); b[2] = div(-x[2], b[0]); b[3] = div(-x[3], b[0])
        else:
            b[0] = sqrt(x[0]); b[1] = div(x[1], b[0]); b[2] = div(x[2], b[0]); b[3] = div(x[3], b[0])
        return b
    if x[0] < 0:
        b[0] = sqrt(-x[0]); b[1] = sqrt(-x[2]) if x[2] < 0 else 0.0
    else:
        b[0] = sqrt(x[0]); b[1] = sqrt(x[2]) if x[2] > 0 else 0.0
    if x[1] < 0:
        b[0] = -b[0]
    if approx == 3:
        b[2] = div(x[3], b[0])
    return b


def gauss_newton(L, rho, b):
    x = [0.0] * 4
    for _ in range(5):
        A, B = [0.0] * 24, [0.0] * 6
        for i in range(6):
            r = L[i]
            A[i * 4 + 0] = 2 * r[0] * b[0] + r[1] * b[1] + r[3] * b[2] + r[6] * b[3]
            A[i * 4 + 1] = r[1] * b[0] + 2 * r[2] * b[1] + r[4] * b[2] + r[7] * b[3]
            A[i * 4 + 2] = r[3] * b[0] + r[4] * b[1] + 2 * r[5] * b[2] + r[8] * b[3]
            A[i * 4 + 3] = r[6] * b[0] + r[7] * b[1] + r[8] * b[2] + 2 * r[9] * b[3]
            B[i] = rho[i] - (r[0] * b[0] * b[0] + r[1] * b[0] * b[1] + r[2] * b[1] * b[1] + r[3] * b[0] * b[2] + r[4] * b[1] * b[2] +
                             r[5] * b[2] * b[2] + r[6] * b[0] * b[3] + r[7] * b[1] * b[3] + r[8] * b[2] * b[3] + r[9] * b[3] * b[3])
        qr_solve(A, B, x)
        for i in range(4):
            b[i] += x[i]


def compute_pose(pws, us, K):
    """compute_pose (:477-525): pws [np, 3], us [np, 2] float64 -> (R [3][3], t [3], approximation 1-3, rep_errors [3])"""
    pws, us = np.asarray(pws, f64), np.asarray(us, f64)
    npts = len(pws)
    dn = float(npts)
    fu, fv, uc, vc = (float(f32(k)) for k in K)
    with np.errstate(all="ignore"):
        cws = [[div(float(s), dn) for s in seqsum(pws)]]
        c0 = np.array(cws[0])
        d = pws - c0
        P = [[0.0] * 3 for _ in range(3)]
        for a in range(3):
            for b in range(a, 3):
                P[a][b] = P[b][a] = float(seqsum(d[:, a] * d[:, b]))
        dc, uct = eig_sym(P)
        for i in range(1, 4):
            k = sqrt(div(dc[i - 1], dn))
            cws.append([cws[0][j] + k * uct[i - 1][j] for j in range(3)])
        cc = [[cws[j][i] - cws[0][i] for j in range(1, 4)] for i in range(3)]
        ci = svd_invert3(cc)
        al = np.zeros((npts, 4))
        for j in range(3):
            al[:, 1 + j] = ci[j][0] * d[:, 0] + ci[j][1] * d[:, 1] + ci[j][2] * d[:, 2]
        al[:, 0] = 1.0 - al[:, 1] - al[:, 2] - al[:, 3]
        # M: rows 2 i (M1) and 2 i + 1 (M2)
        M = np.zeros((npts, 2, 12))
        du, dv = uc - us[:, 0], vc - us[:, 1]
        for k in range(4):
            M[:, 0, 3 * k] = al[:, k] * fu
            M[:, 0, 3 * k + 2] = al[:, k] * du
            M[:, 1, 3 * k + 1] = al[:, k] * fv
            M[:, 1, 3 * k + 2] = al[:, k] * dv
        M = M.reshape(2 * npts, 12)
        MtM = [[0.0] * 12 for _ in range(12)]
        for r in range(12):
            prods = M[:, r:r + 1] * M[:, r:]
            sums = seqsum(prods)
            for c in range(r, 12):
                MtM[r][c] = MtM[c][r] = float(sums[c - r])
        _, ut = eig_sym(MtM)
        v = [ut[11 - i] for i in range(4)]
        L = [[0.0] * 10 for _ in range(6)]
        a, b = 0, 1
        for j in range(6):
            dvv = [[v[i][3 * a + k] - v[i][3 * b + k] for k in range(3)] for i in range(4)]
            L[j] = [dot(dvv[0], dvv[0]), 2.0 * dot(dvv[0], dvv[1]), dot(dvv[1], dvv[1]), 2.0 * dot(dvv[0], dvv[2]), 2.0 * dot(dvv[1], dvv[2]),
                    dot(dvv[2], dvv[2]), 2.0 * dot(dvv[0], dvv[3]), 2.0 * dot(dvv[1], dvv[3]), 2.0 * dot(dvv[2], dvv[3]), dot(dvv[3], dvv[3])]
            b += 1
            if b > 3:
                a += 1
                b = a + 1
        rho = [dist2(cws[0], cws[1]), dist2(cws[0], cws[2]), dist2(cws[0], cws[3]), dist2(cws[1], cws[2]), dist2(cws[1], cws[3]), dist2(cws[2], cws[3])]
        Rs, ts, rep = [], [], []
        for ap in (1, 2, 3):
            betas = find_betas(L, rho, ap)
            gauss_newton(L, rho, betas)
            ccs = [0.0] * 12
            for i in range(4):
                for k in range(12):
                    ccs[k] += betas[i] * v[i][k]
            pcs = np.zeros((npts, 3))
            for j in range(3):
                pcs[:, j] = al[:, 0] * ccs[j] + al[:, 1] * ccs[3 + j] + al[:, 2] * ccs[6 + j] + al[:, 3] * ccs[9 + j]
            if pcs[0, 2] < 0.0:
                pcs = -pcs
            pc0 = [div(float(s), dn) for s in seqsum(pcs)]
            pw0 = [div(float(s), dn) for s in seqsum(pws)]
            dpc, dpw = pcs - np.array(pc0), pws - np.array(pw0)
            abt = [[float(seqsum(dpc[:, j] * dpw[:, c])) for c in range(3)] for j in range(3)]
            U, V, _ = svd3_d(abt)
            R = [[dot(U[i], V[j]) for j in range(3)] for i in range(3)]
            det = (R[0][0] * R[1][1] * R[2][2] + R[0][1] * R[1][2] * R[2][0] + R[0][2] * R[1][0] * R[2][1] -
                   R[0][2] * R[1][1] * R[2][0] - R[0][1] * R[1][0] * R[2][2] - R[0][0] * R[1][2] * R[2][1])
            if det < 0:
                R[2] = [-R[2][0], -R[2][1], -R[2][2]]
            t = [pc0[0] - dot(R[0], pw0), pc0[1] - dot(R[1], pw0), pc0[2] - dot(R[2], pw0)]
            Xc = (R[0][0] * pws[:, 0] + R[0][1] * pws[:, 1] + R[0][2] * pws[:, 2]) + t[0]
            Yc = (R[1][0] * pws[:, 0] + R[1][1] * pws[:, 1] + R[1][2] * pws[:, 2]) + t[1]
            inv_Zc = 1.0 / ((R[2][0] * pws[:, 0] + R[2][1] * pws[:, 1] + R[2][2] * pws[:, 2]) + t[2])
            ue, ve = uc + fu * Xc * inv_Zc, vc + fv * Yc * inv_Zc
            terms = np.sqrt((us[:, 0] - ue) * (us[:, 0] - ue) + (us[:, 1] - ve) * (us[:, 1] - ve))
            rep.append(div(float(seqsum(terms)), dn))
            Rs.append(R); ts.append(t)
        N = 1
        if rep[1] < rep[0]:
            N = 2
        if rep[2] < rep[N - 1]:
            N = 3
    return Rs[N - 1], ts[N - 1], N, rep


def errors(corrs, R, t, K):
    """CheckInliers (:308-339) -> (error2 [n] float32, threshold inputs are the caller's)"""
    fu, fv, uc, vc = (f64(f32(k)) for k in K)
    w = corrs["w"].astype(f64)
    with np.errstate(all="ignore"):
        Xc = (R[0][0] * w[:, 0] + R[0][1] * w[:, 1] + R[0][2] * w[:, 2] + t[0]).astype(f32)
        Yc = (R[1][0] * w[:, 0] + R[1][1] * w[:, 1] + R[1][2] * w[:, 2] + t[1]).astype(f32)
        invZc = (1.0 / (R[2][0] * w[:, 0] + R[2][1] * w[:, 1] + R[2][2] * w[:, 2] + t[2])).astype(f32)
        ue = uc + fu * Xc.astype(f64) * invZc.astype(f64)
        ve = vc + fv * Yc.astype(f64) * invZc.astype(f64)
        dx = (corrs["u"].astype(f64) - ue).astype(f32)
        dy = (corrs["v"].astype(f64) - ve).astype(f32)
        return (dx * dx + dy * dy).astype(f32)


def tcw(R, t):
    T = np.zeros((4, 4), f32)
    with np.errstate(all="ignore"):
        T[:3, :3] = np.array(R, f64).astype(f32)
        T[:3, 3] = np.array(t, f64).astype(f32)
    T[3, 3] = 1
    return T


def model(corrs, idx, K, th2):
    """EPnP on corrs[idx] and CheckInliers over all -> dict(m [12] float64, Tcw, choice, err [n], thr [n], flags [n], count)"""
    pts = corrs[idx]
    R, t, N, rep = compute_pose(pts["w"].astype(f64), np.stack([pts["u"], pts["v"]], axis=1).astype(f64), K)
    err = errors(corrs, R, t, K)
    thr = (corrs["sigma2"] * f32(th2)).astype(f32)
    with np.errstate(invalid="ignore"):
        flags = (err < thr).astype(np.uint8)
    return dict(m=np.array([x for r in R for x in r] + list(t), f64), Tcw=tcw(R, t), choice=N, err=err, thr=thr, flags=flags,
                count=int(flags.sum()), rep=rep)


def replay(counts, rcounts, min_inliers, max_iterations, iterations_done, prior_best):
    """k_pnp_select's loop: the refined count is looked up at the slot of the best set (slot len(counts) = the prior set)
    -> dict(hit_iteration, iterations_run, best_iteration, best_inliers, refined_inliers, no_more, pose, slot)"""
    its = len(counts)
    o = dict(hit_iteration=-1, iterations_run=0, best_iteration=-1, best_inliers=prior_best, refined_inliers=0, no_more=0, pose=POSE_NONE, slot=-2)
    best, best_it = prior_best, -1
    for it in range(its):
        o["iterations_run"] += 1
        c = int(counts[it])
        if c >= min_inliers:
            if c > best:
                best, best_it = c, it
            slot = its if best_it < 0 else best_it
            if rcounts[slot] > min_inliers:
                o.update(hit_iteration=it, refined_inliers=int(rcounts[slot]), pose=POSE_REFINED, slot=slot)
                break
    o.update(best_iteration=best_it, best_inliers=best)
    if o["hit_iteration"] < 0 and iterations_done + o["iterations_run"] >= max_iterations:
        o["no_more"] = 1
        if best >= min_inliers:
            o["pose"] = POSE_BEST if best_it >= 0 else POSE_PRIOR_BEST
            o["slot"] = best_it
    return o


def records(counts, min_inliers, prior_best):
    """the slots k_pnp_refine computes: strict prefix maxima >= min_inliers and above the prior best count"""
    out, top = [], -1
    for it, c in enumerate(counts):
        if c >= min_inliers and c > prior_best and c > top:
            out.append(it)
        top = max(top, int(c))
    return out


def ransac(corrs, K, th2, min_inliers, max_iterations, sets, iterations_done=0, prior_best_inliers=0, prior_best_flags=None):
    """one problem: what orbp_pnp_ransac returns, plus the trace (err, thr per iteration and per computed slot)"""
    corrs = np.asarray(corrs, CORR_DTYPE)
    sets = np.asarray(sets, np.int32).reshape(-1, 4)
    n, its = len(corrs), len(sets)
    prior = np.zeros(n, np.uint8) if prior_best_flags is None else np.asarray(prior_best_flags, np.uint8)
    out = dict(n=n, iterations=its, counts=np.zeros(its, np.int32), models=np.zeros((its, 12)), tcws=np.zeros((its, 4, 4), f32),
               choices=np.zeros(its, np.int32), flags=np.zeros((its, n), np.uint8), err=np.zeros((its, n), f32), rep=np.zeros(its),
               rcounts=np.full(its + 1, -1, np.int32), rmodels=np.zeros((its + 1, 12)), rtcws=np.zeros((its + 1, 4, 4), f32),
               rflags=np.zeros((its + 1, n), np.uint8), rerr=np.full((its + 1, n), np.nan, f32), thr=(corrs["sigma2"] * f32(th2)).astype(f32))
    live = n >= min_inliers and its > 0
    if live:
        for it in range(its):
            m = model(corrs, sets[it], K, th2)
            out["counts"][it], out["models"][it], out["tcws"][it], out["choices"][it] = m["count"], m["m"], m["Tcw"], m["choice"]
            out["flags"][it], out["err"][it], out["rep"][it] = m["flags"], m["err"], m["rep"][m["choice"] - 1]
        slots = records(out["counts"], min_inliers, prior_best_inliers) + ([its] if prior_best_inliers > 0 else [])
        for s in slots:
            src = prior if s == its else out["flags"][s]
            m = model(corrs, np.nonzero(src)[0], K, th2)
            out["rcounts"][s], out["rmodels"][s], out["rtcws"][s], out["rflags"][s], out["rerr"][s] = m["count"], m["m"], m["Tcw"], m["flags"], m["err"]
        o = replay(out["counts"], out["rcounts"], min_inliers, max_iterations, iterations_done, prior_best_inliers)
    else:
        o = dict(hit_iteration=-1, iterations_run=0, best_iteration=-1, best_inliers=prior_best_inliers, refined_inliers=0, no_more=1,
                 pose=POSE_NONE, slot=-2)
    out.update(o)
    zero = np.zeros(n, np.uint8)
    bi = o["best_iteration"]
    out["best_Tcw"] = out["tcws"][bi] if bi >= 0 else np.zeros((4, 4), f32)
    out["best_flags"] = out["flags"][bi] if bi >= 0 else (prior if prior_best_inliers > 0 else zero)
    if o["pose"] == POSE_REFINED:
        out["Tcw"], out["inliers"] = out["rtcws"][o["slot"]], out["rflags"][o["slot"]]
    elif o["pose"] in (POSE_BEST, POSE_PRIOR_BEST):
        out["Tcw"], out["inliers"] = out["best_Tcw"], (out["flags"][bi] if bi >= 0 else prior)
    else:
        out["Tcw"], out["inliers"] = np.zeros((4, 4), f32), zero
    return out


def pnp_parameters(n, probability=0.99, min_inliers=8, max_iterations=300, min_set=4, epsilon=0.4):
    """SetRansacParameters (:121-157) -> (adjusted min_inliers, adjusted max_iterations)"""
    eps = f32(epsilon)
    nmin = int(f32(n) * eps)
    nmin = max(nmin, min_inliers, min_set)
    with np.errstate(all="ignore"):
        r = f32(nmin) / f32(n)
    if eps < r:
        eps = r
    if nmin == n:
        k = 1
    else:
        e = float(eps)
        arg = 1 - math.pow(e, 3)                                     # pow(inf, 3) = inf; log of a negative number is NaN
        den = math.log(arg) if arg > 0 else (-math.inf if arg == 0 else NAN)
        q = div(math.log(1 - probability), den)
        k = max_iterations if not (q <= max_iterations - 1) else (1 if q < 1 else int(math.ceil(q)))
    return nmin, max(1, min(k, max_iterations))


def draw_sets(n, iterations, randint):
    """:188-201: per iteration 4 distinct indices < n without replacement - the drawn slot is overwritten by the last available
    index, which is dropped.  randint(lo, hi) is inclusive, as DUtils::Random::RandomInt."""
    sets = np.zeros((iterations, 4), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(4):
            k = randint(0, len(avail) - 1)
            sets[it, j] = avail[k]
            avail[k] = avail[-1]
            avail.pop()
    return sets


def iterate_reference(counts, refine_of, min_inliers, max_iterations, n_iterations, state):
    """A direct transcription of PnPsolver::iterate / Refine (:165-305) over given counts: refines at EVERY qualifying iteration, as
    the reference does.  refine_of(key) -> refined count of the set `key` (an iteration index of this call, or "prior").
    state: dict(done, best, best_key).  -> (hit iteration or -1, iterations run, no_more, returns_best)"""
    run, cur = 0, 0
    while state["done"] < max_iterations or cur < n_iterations:
        if run >= len(counts):
            raise AssertionError("the call runs more iterations than it was given")
        cur += 1
        state["done"] += 1
        c = counts[run]
        run += 1
        if c >= min_inliers:
            if c > state["best"]:
                state["best"], state["best_key"] = c, run - 1
            if refine_of(state["best_key"]) > min_inliers:
                return run - 1, run, False, False
    if state["done"] >= max_iterations:
        return -1, run, True, state["best"] >= min_inliers
    return -1, run, False, False
