"""Initializer::Initialize (src/Initializer.cc:44-929) restated in numpy, operation by operation as csrc/orbx_initializer.hip and
csrc/orbx_jacobi_svd.h compute it: float32 where the reference is CV_32F, float64 where it promotes, the same Jacobi SVD, the same
orders of summation (np.add.accumulate is sequential).  Hypotheses, matches and motions are batched along numpy axes; an element's
arithmetic does not depend on the batch.  tests/test_initializer_cpu.py checks it against ground truth and, byte for byte, against
the kernels' text compiled for the host; tests/test_initializer_gpu.py compares the device with it.

  search(...)       FindHomography + FindFundamental: all scores, the winners, their inliers, the margins of the winners' matches
  initialize(...)   the whole call -> dict with result, R21, t21, P3D, triangulated, info fields and a trace
  draw_sets         the reference's procedure for mvSets (:78-97) over any inclusive randint
"""
import ctypes
import ctypes.util

import numpy as np

F32, F64 = np.float32, np.float64
JS_MAX_SWEEPS = 30
JS_EPS = 2.0 * float(np.finfo(np.float32).eps)
CV_PI = 3.1415926535897932384626433832795
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.acosf.restype = ctypes.c_float
_libm.acosf.argtypes = [ctypes.c_float]


def acosf(x):
    """libm's float acos: the one function on the path that is not +, -, *, / or sqrt"""
    return F32(_libm.acosf(float(x)))


def seq_sum(x, axis):
    """sum along axis in ascending order, one accumulator of x's dtype"""
    return np.take(np.add.accumulate(x, axis=axis, dtype=x.dtype), -1, axis=axis)


def jacobi_sweeps(W, M):
    """W [B, M + N, N] float32, in place (csrc/orbx_jacobi_svd.h: jacobi_sweeps)"""
    N = W.shape[2]
    with np.errstate(all="ignore"):
        for _ in range(JS_MAX_SWEEPS):
            changed = False
            for p in range(N - 1):
                for q in range(p + 1, N):
                    x, y = W[:, :M, p].astype(F64), W[:, :M, q].astype(F64)
                    a, b, g = seq_sum(x * x, 1), seq_sum(y * y, 1), seq_sum(x * y, 1)
                    rot = np.abs(g) > JS_EPS * np.sqrt(a * b)
                    if not rot.any():
                        continue
                    changed = True
                    g2 = 2.0 * g
                    beta = a - b
                    gamma = np.sqrt(g2 * g2 + beta * beta)
                    s_n = np.sqrt(((gamma - beta) * 0.5) / gamma)
                    c_n = g2 / ((gamma * s_n) * 2.0)
                    c_p = np.sqrt((gamma + beta) / (gamma * 2.0))
                    s_p = g2 / ((gamma * c_p) * 2.0)
                    neg = beta < 0.0
                    cf = np.where(neg, c_n, c_p).astype(F32)[:, None]
                    sf = np.where(neg, s_n, s_p).astype(F32)[:, None]
                    X, Y = W[:, :, p].copy(), W[:, :, q].copy()
                    W[:, :, p] = np.where(rot[:, None], cf * X + sf * Y, X)
                    W[:, :, q] = np.where(rot[:, None], cf * Y - sf * X, Y)
            if not changed:
                break


def jacobi_order(W, M):
    """-> w [B, N] float32 (unsorted), order [B, N]: columns by descending w, stable"""
    B, _, N = W.shape
    x = W[:, :M, :].astype(F64)
    with np.errstate(all="ignore"):
        w = np.sqrt(seq_sum(x * x, 1)).astype(F32)
    order = np.zeros((B, N), np.int64)
    for e in range(B):
        used = [False] * N
        for k in range(N):
            best = -1
            for j in range(N):
                if not used[j] and (best < 0 or w[e, j] > w[e, best]):
                    best = j
            used[best] = True
            order[e, k] = best
    return w, order


def svd3(A):
    """A [B, 3, 3] float32 -> w [B, 3], U, Vt [B, 3, 3]"""
    B = A.shape[0]
    W = np.concatenate([A.astype(F32), np.broadcast_to(np.eye(3, dtype=F32), (B, 3, 3))], axis=1).copy()
    jacobi_sweeps(W, 3)
    wu, order = jacobi_order(W, 3)
    e = np.arange(B)
    w = np.stack([wu[e, order[:, k]] for k in range(3)], axis=1)
    Vt = np.stack([W[e, 3:, order[:, k]] for k in range(3)], axis=1)            # row k = column order[k] of V
    U = np.zeros((B, 3, 3), F32)
    with np.errstate(all="ignore"):
        for k in range(2):
            U[:, :, k] = W[e, :3, order[:, k]] / w[:, k, None]
        u0, u1 = U[:, :, 0], U[:, :, 1]
        u2 = np.stack([u0[:, 1] * u1[:, 2] - u0[:, 2] * u1[:, 1], u0[:, 2] * u1[:, 0] - u0[:, 0] * u1[:, 2],
                       u0[:, 0] * u1[:, 1] - u0[:, 1] * u1[:, 0]], axis=1)
        d = seq_sum(u2.astype(F64) * W[e, :3, order[:, 2]].astype(F64), 1)
    U[:, :, 2] = np.where((d < 0.0)[:, None], -u2, u2)
    return w, U, Vt


def svd4_null(A):
    """A [B, 4, 4] float32 -> x [B, 4]: the right singular vector of the smallest singular value"""
    B = A.shape[0]
    W = np.concatenate([A.astype(F32), np.broadcast_to(np.eye(4, dtype=F32), (B, 4, 4))], axis=1).copy()
    jacobi_sweeps(W, 4)
    _, order = jacobi_order(W, 4)
    return W[np.arange(B), 4:, order[:, 3]]


def gemm(a, b, alpha=1.0):
    """cv::gemm on CV_32F with an inner dimension of 3: double accumulation left to right, x alpha, narrowed"""
    prod = a.astype(F64)[..., :, :, None] * b.astype(F64)[..., None, :, :]
    return (((prod[..., 0, :] + prod[..., 1, :]) + prod[..., 2, :]) * F64(alpha)).astype(F32)


def det3(m):
    m = m.astype(F64)
    return (m[..., 0, 0] * (m[..., 1, 1] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 1])
            - m[..., 0, 1] * (m[..., 1, 0] * m[..., 2, 2] - m[..., 1, 2] * m[..., 2, 0])
            + m[..., 0, 2] * (m[..., 1, 0] * m[..., 2, 1] - m[..., 1, 1] * m[..., 2, 0]))


def invert33(mf):
    """cv::invert(DECOMP_LU) on 3x3 CV_32F; singular: zeros"""
    d = det3(mf)
    m = mf.astype(F64)
    with np.errstate(all="ignore"):
        di = 1.0 / d
    M = lambda i, j: m[..., i, j]   # noqa: E731
    t = np.stack([(M(1, 1) * M(2, 2) - M(1, 2) * M(2, 1)) * di, (M(0, 2) * M(2, 1) - M(0, 1) * M(2, 2)) * di,
                  (M(0, 1) * M(1, 2) - M(0, 2) * M(1, 1)) * di, (M(1, 2) * M(2, 0) - M(1, 0) * M(2, 2)) * di,
                  (M(0, 0) * M(2, 2) - M(0, 2) * M(2, 0)) * di, (M(0, 2) * M(1, 0) - M(0, 0) * M(1, 2)) * di,
                  (M(1, 0) * M(2, 1) - M(1, 1) * M(2, 0)) * di, (M(0, 1) * M(2, 0) - M(0, 0) * M(2, 1)) * di,
                  (M(0, 0) * M(1, 1) - M(0, 1) * M(1, 0)) * di], axis=-1)
    t = np.where((d == 0.0)[..., None], 0.0, t)
    return t.astype(F32).reshape(m.shape)


def norm3(v):
    v = v.astype(F64)
    return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])


def normalize(keys):
    """Normalize (:749-795) over all keys -> mean [2], scale [2], T [3, 3]"""
    keys = np.ascontiguousarray(keys, F32)
    n = F32(len(keys))
    mean = np.array([seq_sum(keys[:, 0], 0) / n, seq_sum(keys[:, 1], 0) / n], F32)
    dev = np.abs(keys - mean[None, :])
    mdev = np.array([seq_sum(dev[:, 0], 0) / n, seq_sum(dev[:, 1], 0) / n], F32)
    with np.errstate(all="ignore"):
        sc = (1.0 / mdev.astype(F64)).astype(F32)
    T = np.array([[sc[0], 0, -mean[0] * sc[0]], [0, sc[1], -mean[1] * sc[1]], [0, 0, 1]], F32)
    return mean, sc, T


def search(keys1, keys2, matches, sets, sigma=1.0):
    keys1, keys2 = np.ascontiguousarray(keys1, F32).reshape(-1, 2), np.ascontiguousarray(keys2, F32).reshape(-1, 2)
    matches, sets = np.asarray(matches, np.int64).reshape(-1, 2), np.asarray(sets, np.int64).reshape(-1, 8)
    N, iters = len(matches), len(sets)
    sigma = F32(sigma)
    mean1, sc1, T1 = normalize(keys1)
    mean2, sc2, T2 = normalize(keys2)
    T2inv, T2t = invert33(T2), T2.T.copy()
    p1, p2 = keys1[matches[:, 0]], keys2[matches[:, 1]]
    n1 = (p1[sets] - mean1) * sc1          # [iters, 8, 2]
    n2 = (p2[sets] - mean2) * sc2
    u1, v1, u2, v2 = n1[..., 0], n1[..., 1], n2[..., 0], n2[..., 1]
    z, o = np.zeros_like(u1), np.ones_like(u1)
    WH = np.zeros((iters, 25, 9), F32)
    WH[:, 0:16:2, :] = np.stack([z, z, z, -u1, -v1, -o, v2 * u1, v2 * v1, v2], axis=-1)
    WH[:, 1:16:2, :] = np.stack([u1, v1, o, z, z, z, -u2 * u1, -u2 * v1, -u2], axis=-1)
    WF = np.zeros((iters, 25, 9), F32)
    WF[:, 0:8, :] = np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, o], axis=-1)
    W = np.concatenate([WH, WF])
    W[:, 16:, :] = np.eye(9, dtype=F32)
    jacobi_sweeps(W, 16)
    _, order = jacobi_order(W, 16)
    Mn = W[np.arange(2 * iters), 16:, order[:, 8]].reshape(2 * iters, 3, 3)
    H21 = gemm(gemm(T2inv, Mn[:iters]), T1)
    H12 = invert33(H21)
    wf, U, Vt = svd3(Mn[iters:])
    D = np.zeros((iters, 3, 3), F32)
    D[:, 0, 0], D[:, 1, 1] = wf[:, 0], wf[:, 1]
    Fn = gemm(gemm(U, D), Vt)
    F21 = gemm(gemm(T2t, Fn), T1)

    x1, y1, x2, y2 = (a[None, :] for a in (p1[:, 0], p1[:, 1], p2[:, 0], p2[:, 1]))
    inv_s2 = F32(1.0 / F64(sigma * sigma))
    thH, thF, thScore = F32(5.991), F32(3.841), F32(5.991)
    with np.errstate(all="ignore"):
        h, g = H21.reshape(iters, 9, 1), H12.reshape(iters, 9, 1)
        w2 = (1.0 / (g[:, 6] * x2 + g[:, 7] * y2 + g[:, 8]).astype(F64)).astype(F32)
        ua, va = (g[:, 0] * x2 + g[:, 1] * y2 + g[:, 2]) * w2, (g[:, 3] * x2 + g[:, 4] * y2 + g[:, 5]) * w2
        chiH1 = ((x1 - ua) * (x1 - ua) + (y1 - va) * (y1 - va)) * inv_s2
        w1 = (1.0 / (h[:, 6] * x1 + h[:, 7] * y1 + h[:, 8]).astype(F64)).astype(F32)
        ub, vb = (h[:, 0] * x1 + h[:, 1] * y1 + h[:, 2]) * w1, (h[:, 3] * x1 + h[:, 4] * y1 + h[:, 5]) * w1
        chiH2 = ((x2 - ub) * (x2 - ub) + (y2 - vb) * (y2 - vb)) * inv_s2
        f = F21.reshape(iters, 9, 1)
        a2, b2, c2 = f[:, 0] * x1 + f[:, 1] * y1 + f[:, 2], f[:, 3] * x1 + f[:, 4] * y1 + f[:, 5], f[:, 6] * x1 + f[:, 7] * y1 + f[:, 8]
        num2 = a2 * x2 + b2 * y2 + c2
        chiF1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2
        a1, b1, c1 = f[:, 0] * x2 + f[:, 3] * y2 + f[:, 6], f[:, 1] * x2 + f[:, 4] * y2 + f[:, 7], f[:, 2] * x2 + f[:, 5] * y2 + f[:, 8]
        num1 = a1 * x1 + b1 * y1 + c1
        chiF2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2

        def score(c1_, c2_, th, ths):
            o1, o2 = c1_ > th, c2_ > th
            terms = np.empty((iters, 2 * N), F32)
            terms[:, 0::2] = np.where(o1, F32(0), ths - c1_)
            terms[:, 1::2] = np.where(o2, F32(0), ths - c2_)
            return seq_sum(terms, 1), ~(o1 | o2)
        sH, inH = score(chiH1, chiH2, thH, thH)
        sF, inF = score(chiF1, chiF2, thF, thScore)

    def first_best(s):
        best, bi = F32(0), -1
        for it in range(iters):
            if s[it] > best:
                best, bi = s[it], it
        return best, bi
    SH, bH = first_best(sH)
    SF, bF = first_best(sF)

    def margin(chis, th, b):
        if b < 0:
            return np.inf
        with np.errstate(all="ignore"):
            m = np.abs(np.stack([c[b] for c in chis]).astype(F64) / F64(th) - 1.0)
        return float(np.nanmin(m)) if np.isfinite(m).any() else np.inf
    return dict(scores=np.stack([sH, sF]), SH=SH, SF=SF, best=(bH, bF),
                H21=H21[bH] if bH >= 0 else np.zeros((3, 3), F32), F21=F21[bF] if bF >= 0 else np.zeros((3, 3), F32),
                inliersH=inH[bH] if bH >= 0 else np.zeros(N, bool), inliersF=inF[bF] if bF >= 0 else np.zeros(N, bool),
                margin_chi=min(margin((chiH1, chiH2), thH, bH), margin((chiF1, chiF2), thF, bF)), T1=T1, T2=T2, p1=p1, p2=p2)


def check_rt(R, t, p1, p2, inl, K4, th2):
    """CheckRT (:798-907) for C motions at once: R [C, 3, 3], t [C, 3] -> nGood [C], parallax [C], P3D [C, N, 3], flags [C, N] (bit 1
    counted, bit 0 vbGood), margin: the smallest relative distance of a comparison that was reached from its threshold"""
    fx, fy, cx, cy = (F32(v) for v in K4)
    C, N = len(R), len(p1)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F32)
    P1 = np.concatenate([K, np.zeros((3, 1), F32)], axis=1)
    P2 = gemm(K, np.concatenate([R, t[:, :, None]], axis=2))                       # [C, 3, 4]
    O2 = gemm(np.swapaxes(R, 1, 2), t[:, :, None], -1.0)[:, :, 0]                  # [C, 3]
    idx = np.nonzero(inl)[0]
    x1, y1, x2, y2 = (a[None, :, None] for a in (p1[idx, 0], p1[idx, 1], p2[idx, 0], p2[idx, 1]))
    n = len(idx)
    A = np.empty((C, n, 4, 4), F32)
    A[:, :, 0, :] = x1 * P1[None, None, 2, :] - P1[None, None, 0, :]
    A[:, :, 1, :] = y1 * P1[None, None, 2, :] - P1[None, None, 1, :]
    A[:, :, 2, :] = x2 * P2[:, None, 2, :] - P2[:, None, 0, :]
    A[:, :, 3, :] = y2 * P2[:, None, 2, :] - P2[:, None, 1, :]
    x = svd4_null(A.reshape(C * n, 4, 4)).reshape(C, n, 4)
    x1, y1, x2, y2 = (a[:, :, 0] for a in (x1, y1, x2, y2))
    th2 = F32(th2)
    with np.errstate(all="ignore"):
        p = (x[..., :3].astype(F64) * (1.0 / x[..., 3].astype(F64))[..., None]).astype(F32)
        alive = np.isfinite(p).all(axis=2)
        dist1 = norm3(p).astype(F32)
        nrm2 = p - O2[:, None, :]
        dist2 = norm3(nrm2).astype(F32)
        pd, nd = p.astype(F64), nrm2.astype(F64)
        dot = (pd[..., 0] * nd[..., 0] + pd[..., 1] * nd[..., 1]) + pd[..., 2] * nd[..., 2]
        cosP = (dot / (dist1 * dist2).astype(F64)).astype(F32)
        low = cosP.astype(F64) < 0.99998
        mcos, alive0 = np.abs(cosP.astype(F64) / 0.99998 - 1.0), alive.copy()
        alive &= ~((p[..., 2] <= 0) & low)
        Rd, td = R.astype(F64)[:, None], t.astype(F64)[:, None]
        q = (((Rd[..., 0] * pd[..., None, 0] + Rd[..., 1] * pd[..., None, 1]) + Rd[..., 2] * pd[..., None, 2]) + td).astype(F32)
        behind = alive0 & ((p[..., 2] <= 0) | (alive & (q[..., 2] <= 0)))      # where the && reaches the 0.99998 comparison
        alive &= ~((q[..., 2] <= 0) & low)
        margins = []
        iz1 = (1.0 / p[..., 2].astype(F64)).astype(F32)
        e1x, e1y = (fx * p[..., 0] * iz1 + cx) - x1, (fy * p[..., 1] * iz1 + cy) - y1
        se1 = e1x * e1x + e1y * e1y
        margins.append(np.where(alive, np.abs(se1.astype(F64) / F64(th2) - 1.0), np.inf))
        alive &= ~(se1 > th2)
        iz2 = (1.0 / q[..., 2].astype(F64)).astype(F32)
        e2x, e2y = (fx * q[..., 0] * iz2 + cx) - x2, (fy * q[..., 1] * iz2 + cy) - y2
        se2 = e2x * e2x + e2y * e2y
        margins.append(np.where(alive, np.abs(se2.astype(F64) / F64(th2) - 1.0), np.inf))
        alive &= ~(se2 > th2)
        margins.append(np.where(behind | alive, mcos, np.inf))                  # ... and the vbGood test of a counted point
    P3D, flags = np.zeros((C, N, 3), F32), np.zeros((C, N), np.uint8)
    nGood, par = alive.sum(axis=1), np.zeros(C, F32)
    for c in range(C):
        P3D[c, idx[alive[c]]] = p[c, alive[c]]
        flags[c, idx[alive[c]]] = 2 | low[c, alive[c]].astype(np.uint8)
        if nGood[c] > 0:
            v = np.sort(cosP[c, alive[c]])[min(50, nGood[c] - 1)]
            par[c] = F32(F64(acosf(v) * F32(180)) / CV_PI)
    m = np.stack(margins)                                                       # [error 1, error 2, cos][C, n]
    m = np.where(np.isnan(m), np.inf, m)
    check_rt.last_margins = m
    return nGood.astype(int), par, P3D, flags, float(m.min()) if m.size else np.inf


def initialize(keys1, keys2, matches, sets, K4, sigma=1.0, min_parallax=1.0, min_triangulated=50):
    s = search(keys1, keys2, matches, sets, sigma)
    N = len(s["p1"])
    sigma, minPar = F32(sigma), F32(min_parallax)
    fx, fy, cx, cy = (F32(v) for v in K4)
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], F32)
    with np.errstate(all="ignore"):
        RH = s["SH"] / (s["SH"] + s["SF"])
    model = 0 if RH > F32(0.40) else 1
    inl = s["inliersH"] if model == 0 else s["inliersF"]
    nInl = int(inl.sum())
    r = dict(search=s, SH=s["SH"], SF=s["SF"], RH=RH, model=model, best=s["best"], inliers=(int(s["inliersH"].sum()), int(s["inliersF"].sum())),
             result=0, R21=np.zeros((3, 3), F32), t21=np.zeros(3, F32), P3D=np.zeros((N, 3), F32), triangulated=np.zeros(N, np.uint8),
             best_good=0, second_good=0, parallax=F32(0), ncand=0, ngood=[], cand_parallax=[], margin_rt=np.inf,
             margin_chi=s["margin_chi"], H21=s["H21"], F21=s["F21"], reason="no model")
    if s["best"][model] < 0:
        return r
    Rc = tc = None
    with np.errstate(all="ignore"):
        if model == 0:
            A = gemm(gemm(invert33(K), s["H21"]), K)
            w, U, Vt = (a[0] for a in svd3(A[None]))
            sgn = F32(det3(U) * det3(Vt))
            d1, d2, d3 = w
            r["d"] = (d1, d2, d3)
            if F64(d1 / d2) < 1.00001 or F64(d2 / d3) < 1.00001:
                r["reason"] = "singular values"
                return r
            aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
            aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
            x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
            aux_st = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
            ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
            st = [aux_st, -aux_st, -aux_st, aux_st]
            aux_sp = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
            cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
            sp = [aux_sp, -aux_sp, -aux_sp, aux_sp]
            Rc, tc = np.zeros((8, 3, 3), F32), np.zeros((8, 3), F32)
            for i in range(8):
                j = i & 3
                Rp = np.eye(3, dtype=F32)
                if i < 4:
                    Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ct, -st[j], st[j], ct
                else:
                    Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cp, sp[j], F32(-1), sp[j], -cp
                Rc[i] = gemm(gemm(U, Rp, sgn), Vt)
                tp = np.array([x1[j], F32(0), -x3[j] if i < 4 else x3[j]], F32) * (d1 - d3 if i < 4 else d1 + d3)
                t = gemm(U, tp[:, None])[:, 0]
                tc[i] = (t.astype(F64) * (1.0 / norm3(t))).astype(F32)
        else:
            E = gemm(gemm(K.T.copy(), s["F21"]), K)
            w, U, Vt = (a[0] for a in svd3(E[None]))
            t = U[:, 2].copy()
            t = (t.astype(F64) * (1.0 / norm3(t))).astype(F32)
            Wm = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], F32)
            R1 = gemm(gemm(U, Wm), Vt)
            if det3(R1) < 0:
                R1 = -R1
            R2 = gemm(gemm(U, Wm.T.copy()), Vt)
            if det3(R2) < 0:
                R2 = -R2
            Rc, tc = np.stack([R1, R2, R1, R2]), np.stack([t, t, -t, -t])
    th2 = F32(4.0 * F64(sigma * sigma))
    nG, par, P3D, flags, r["margin_rt"] = check_rt(Rc, tc, s["p1"], s["p2"], inl, K4, th2)
    r["ncand"], r["ngood"], r["cand_parallax"] = len(Rc), [int(g) for g in nG], par
    if model == 0:
        best, second, win, bpar = 0, 0, -1, F32(-1)
        for i in range(8):
            if nG[i] > best:
                second, best, win, bpar = best, nG[i], i, par[i]
            elif nG[i] > second:
                second = nG[i]
        ok = second < 0.75 * best and bpar >= minPar and best > min_triangulated and best > 0.9 * nInl
        r["equalities"] = [second == 0.75 * best, best == min_triangulated, best == 0.9 * nInl]
        r["reason"] = "ok" if ok else ("ambiguous" if not second < 0.75 * best else "parallax" if not bpar >= minPar else "count")
    else:
        best = max(nG)
        nMin = max(int(0.9 * nInl), min_triangulated)
        nsim = sum(1 for g in nG if g > 0.7 * best)
        win = [i for i in range(4) if nG[i] == best][0]
        second = max([nG[i] for i in range(4) if i != win] + [0])
        bpar = par[win]
        ok = not (best < nMin or nsim > 1) and bpar > minPar
        r["equalities"] = [best == nMin] + [g == 0.7 * best for g in nG]
        r["reason"] = "ok" if ok else ("count" if best < nMin else "ambiguous" if nsim > 1 else "parallax")
    r.update(best_good=int(best), second_good=int(second), parallax=F32(bpar), win=win)
    if ok:
        r.update(result=1, R21=Rc[win], t21=tc[win], P3D=P3D[win], triangulated=(flags[win] & 1).astype(np.uint8))
    return r


def draw_sets(n, iterations, randint):
    """mvSets (:78-97): randint(lo, hi) inclusive"""
    sets = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(8):
            k = randint(0, len(avail) - 1)
            sets[it, j] = avail[k]
            avail[k] = avail[-1]
            avail.pop()
    return sets
