"""Sim3Solver (src/Sim3Solver.cc) restated in numpy, operation for operation as csrc/orbx_sim3.hip does it (DESIGN.md section 6,
"k_sim3_*"): hypotheses and pairs are batched along axes; float32 where the reference is CV_32F, float64 where it says double,
cv::gemm as double accumulation left to right narrowed once.  Scalar atan2, sin and cos go through math.* (the C library), as the
lockstep program's do.  cv::eigen is jacobi_eig4 below, cv::Rodrigues is written out: this library's own, not OpenCV's.

perturb = (da, ds, dc): the results of atan2 / sin / cos moved by that many ulp (np.nextafter steps) - what
tests/test_sim3_gpu.py measures the device's math library against."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
PAIR_DTYPE = np.dtype([("w1", "<f4", (3,)), ("w2", "<f4", (3,)), ("sigma2_1", "<f4"), ("sigma2_2", "<f4")])
JE_MAX_SWEEPS = 30
JE_EPS = float(np.finfo(np.float64).eps)


def _d(a):
    return np.asarray(a, f32).astype(f64)


def transform(T, X):
    """Rcw*X+tcw as one cv::gemm: T [..., 4, 4] float32, X [..., 3] float32 -> float32"""
    T, X = _d(T), _d(X)
    return ((((T[..., :3, 0] * X[..., 0:1]) + T[..., :3, 1] * X[..., 1:2]) + T[..., :3, 2] * X[..., 2:3]) + T[..., :3, 3]).astype(f32)


def image(P, K):
    """FromCameraToImage / the tail of Project: invz = 1 / z in float, no guard"""
    P = np.asarray(P, f32)
    fx, fy, cx, cy = (f32(k) for k in K)
    with np.errstate(all="ignore"):
        invz = f32(1) / P[..., 2]
        x, y = P[..., 0] * invz, P[..., 1] * invz
        return np.stack([fx * x + cx, fy * y + cy], axis=-1).astype(f32)


def threshold(sigma2):
    """(size_t)(9.210 * sigmaSquare), truncated, as the float the comparison converts it to"""
    v = 9.210 * _d(sigma2)
    out = np.empty(v.shape, f32)
    big = v >= 18446744073709551616.0
    out[big] = f32(18446744073709551616.0)
    out[~big] = v[~big].astype(np.uint64).astype(f32)
    return out


def prepare(pairs, Tcw1, Tcw2, K1, K2):
    pairs = np.asarray(pairs, PAIR_DTYPE)
    X1c = transform(np.asarray(Tcw1, f32).reshape(4, 4), pairs["w1"]).reshape(-1, 3)
    X2c = transform(np.asarray(Tcw2, f32).reshape(4, 4), pairs["w2"]).reshape(-1, 3)
    return dict(X1c=X1c, X2c=X2c, p1=image(X1c, K1).reshape(-1, 2), p2=image(X2c, K2).reshape(-1, 2),
                thr1=threshold(pairs["sigma2_1"]), thr2=threshold(pairs["sigma2_2"]))


def jacobi_eig4(N):
    """csrc/orbx_jacobi_eig.h: N [H, 4, 4] float32 symmetric -> (eval [H, 4] descending, evec [H, 4, 4], rows the eigenvectors)"""
    N = np.asarray(N, f32).reshape(-1, 4, 4)
    H = len(N)
    A = N.astype(f64)
    V = np.broadcast_to(np.eye(4), (H, 4, 4)).copy()
    ss = np.zeros(H)
    for k in range(16):
        ss = ss + A[:, k // 4, k % 4] * A[:, k // 4, k % 4]
    thr = JE_EPS * np.sqrt(ss)
    with np.errstate(all="ignore"):
        for _ in range(JE_MAX_SWEEPS):
            changed = np.zeros(H, bool)
            for p in range(3):
                for q in range(p + 1, 4):
                    g = A[:, p, q].copy()
                    m = np.abs(g) > thr
                    if not m.any():
                        continue
                    changed |= m
                    theta = (A[:, q, q] - A[:, p, p]) / (2.0 * g)
                    t = 1.0 / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                    t = np.where(theta < 0.0, -t, t)
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    B = A.copy()
                    B[:, p, p] = A[:, p, p] - t * g
                    B[:, q, q] = A[:, q, q] + t * g
                    B[:, p, q] = 0.0
                    B[:, q, p] = 0.0
                    for k in range(4):
                        if k in (p, q):
                            continue
                        x, y = A[:, k, p], A[:, k, q]
                        B[:, k, p] = B[:, p, k] = c * x - s * y
                        B[:, k, q] = B[:, q, k] = s * x + c * y
                    W = V.copy()
                    W[:, :, p] = c[:, None] * V[:, :, p] - s[:, None] * V[:, :, q]
                    W[:, :, q] = s[:, None] * V[:, :, p] + c[:, None] * V[:, :, q]
                    A = np.where(m[:, None, None], B, A)
                    V = np.where(m[:, None, None], W, V)
            if not changed.any():
                break
    ev = np.zeros((H, 4), f32)
    evec = np.zeros((H, 4, 4), f32)
    diag = A[:, np.arange(4), np.arange(4)]
    for h in range(H):
        used = []
        for k in range(4):
            best = -1
            for j in range(4):
                if j not in used and (best < 0 or diag[h, j] > diag[h, best]):
                    best = j
            used.append(best)
            ev[h, k] = f32(diag[h, best])
            evec[h, k] = V[h, :, best].astype(f32)
    return ev, evec


def _nudge(x, ulps):
    for _ in range(abs(int(ulps))):
        x = float(np.nextafter(x, math.inf if ulps > 0 else -math.inf))
    return x


def centroid(P):
    """P [H, 3, 3] float32, the three points in the columns -> (Pr, O): cv::reduce's two accumulators, then * (1./3) in double"""
    s = (P[:, :, 0] + P[:, :, 2]) + P[:, :, 1]
    O = (s.astype(f64) * (1. / 3)).astype(f32)
    return (P - O[:, :, None]).astype(f32), O


def gemm33(A, B):
    A, B = _d(A), _d(B)
    return ((A[..., :, 0:1] * B[..., 0:1, :] + A[..., :, 1:2] * B[..., 1:2, :]) + A[..., :, 2:3] * B[..., 2:3, :]).astype(f32)


def compute_sim3(P1, P2, fix_scale, perturb=(0, 0, 0)):
    """ComputeSim3 for H hypotheses: P1, P2 [H, 3, 3] float32 -> dict(s [H], R [H, 3, 3], t [H, 3], T12, T21 [H, 4, 4])"""
    H = len(P1)
    with np.errstate(all="ignore"):
        Pr1, O1 = centroid(P1)
        Pr2, O2 = centroid(P2)
        M = gemm33(Pr2, np.swapaxes(Pr1, 1, 2))
        m = lambda i, j: M[:, i, j]      # noqa: E731
        N11 = m(0, 0) + m(1, 1) + m(2, 2); N12 = m(1, 2) - m(2, 1); N13 = m(2, 0) - m(0, 2); N14 = m(0, 1) - m(1, 0)
        N22 = m(0, 0) - m(1, 1) - m(2, 2); N23 = m(0, 1) + m(1, 0); N24 = m(2, 0) + m(0, 2)
        N33 = -m(0, 0) + m(1, 1) - m(2, 2); N34 = m(1, 2) + m(2, 1); N44 = -m(0, 0) - m(1, 1) + m(2, 2)
        Nm = np.stack([N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44], axis=1).astype(f32).reshape(H, 4, 4)
        _, evec = jacobi_eig4(Nm)
        vec = evec[:, 0, 1:4].copy()
        v = vec.astype(f64)
        nv = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        R = np.zeros((H, 3, 3), f32)
        for h in range(H):
            ang = _nudge(math.atan2(nv[h], float(evec[h, 0, 0])), perturb[0])
            alpha = (2 * ang) * (np.float64(1.) / nv[h])
            r = (v[h] * alpha).astype(f32).astype(f64)
            theta = math.sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) if np.isfinite(r).all() else float("nan")
            if theta < JE_EPS:                     # DBL_EPSILON; false for NaN
                R[h] = np.eye(3, dtype=f32)
                continue
            if math.isnan(theta) or math.isinf(theta):
                R[h] = np.nan
                continue
            c, s = _nudge(math.cos(theta), perturb[2]), _nudge(math.sin(theta), perturb[1])
            c1 = 1. - c
            k = r / theta
            kk = np.array([[k[0] * k[0], k[0] * k[1], k[0] * k[2]], [k[1] * k[0], k[1] * k[1], k[1] * k[2]], [k[2] * k[0], k[2] * k[1], k[2] * k[2]]])
            Kx = np.array([[0., -k[2], k[1]], [k[2], 0., -k[0]], [-k[1], k[0], 0.]])
            R[h] = ((c * np.eye(3) + c1 * kk) + s * Kx).astype(f32)
        if fix_scale:
            ms = np.ones(H, f32)
        else:
            P3 = gemm33(R, Pr2)
            nom, den = np.zeros(H), np.zeros(H)
            a, b = Pr1.reshape(H, 9).astype(f64), P3.reshape(H, 9)
            for k in range(9):
                nom = nom + a[:, k] * b[:, k].astype(f64)
            for k in range(9):
                den = den + (b[:, k] * b[:, k]).astype(f64)
            ms = (nom / den).astype(f32)
        Rd, sd = R.astype(f64), ms.astype(f64)
        acc = (Rd[:, :, 0] * _d(O2)[:, 0:1] + Rd[:, :, 1] * _d(O2)[:, 1:2]) + Rd[:, :, 2] * _d(O2)[:, 2:3]
        t = (_d(O1) - acc * sd[:, None]).astype(f32)
        T12 = np.zeros((H, 4, 4), f32)
        T21 = np.zeros((H, 4, 4), f32)
        T12[:, :3, :3] = (Rd * sd[:, None, None]).astype(f32)
        T12[:, :3, 3] = t
        inv_s = 1.0 / sd
        T21[:, :3, :3] = (np.swapaxes(Rd, 1, 2) * inv_s[:, None, None]).astype(f32)
        Q, td = T21[:, :3, :3].astype(f64), t.astype(f64)
        T21[:, :3, 3] = (((Q[:, :, 0] * td[:, 0:1] + Q[:, :, 1] * td[:, 1:2]) + Q[:, :, 2] * td[:, 2:3]) * -1.0).astype(f32)
        T12[:, 3, 3] = T21[:, 3, 3] = 1
    return dict(s=ms, R=R, t=t, T12=T12, T21=T21)


def errors(rec, mdl, K1, K2):
    """the two squared reprojection errors of every (hypothesis, pair): float32 [H, n] each"""
    with np.errstate(all="ignore"):
        P2im1 = image(transform(mdl["T12"][:, None], rec["X2c"][None]), K1)
        P1im2 = image(transform(mdl["T21"][:, None], rec["X1c"][None]), K2)
        d1 = (rec["p1"][None] - P2im1).astype(f64)
        d2 = (P1im2 - rec["p2"][None]).astype(f64)
        err1 = (d1[..., 0] * d1[..., 0] + d1[..., 1] * d1[..., 1]).astype(f32)
        err2 = (d2[..., 0] * d2[..., 0] + d2[..., 1] * d2[..., 1]).astype(f32)
    return err1, err2


def select(counts, min_inliers):
    """iterate's loop over stored counts from a fresh solver -> (hit_iteration or -1, best_iteration or -1, best_inliers)"""
    hit, best, best_inl = -1, -1, 0
    for it, c in enumerate(counts):
        if c >= best_inl:
            best_inl, best = int(c), it
            if c > min_inliers:
                hit = it
                break
    return hit, best, best_inl


def ransac(pairs, Tcw1, Tcw2, K1, K2, fix_scale, min_inliers, sets, perturb=(0, 0, 0)):
    """one problem: what orbs_sim3_ransac returns, plus the trace (err1, err2, the record)"""
    sets = np.asarray(sets, np.int32).reshape(-1, 3)
    n, H = len(pairs), len(sets)
    rec = prepare(pairs, Tcw1, Tcw2, K1, K2) if n else None
    out = dict(n=n, iterations=H, rec=rec)
    if H:
        P1 = np.swapaxes(rec["X1c"][sets], 1, 2)      # [H, 3 (set), 3 (xyz)] -> the points in the columns
        P2 = np.swapaxes(rec["X2c"][sets], 1, 2)
        mdl = compute_sim3(np.ascontiguousarray(P1), np.ascontiguousarray(P2), fix_scale, perturb)
        err1, err2 = errors(rec, mdl, K1, K2)
        with np.errstate(invalid="ignore"):
            flags = ((err1 < rec["thr1"][None]) & (err2 < rec["thr2"][None])).astype(np.uint8)
        counts = flags.sum(axis=1).astype(np.int32)
        models = np.concatenate([mdl["s"][:, None], mdl["R"].reshape(H, 9), mdl["t"]], axis=1).astype(f32)
        out.update(err1=err1, err2=err2, T12=mdl["T12"])
    else:
        flags, counts, models = np.zeros((0, n), np.uint8), np.zeros(0, np.int32), np.zeros((0, 13), f32)
    hit, best, best_inl = select(counts, min_inliers)
    out.update(counts=counts, models=models, flags=flags, hit_iteration=hit, best_iteration=best, best_inliers=best_inl,
               hit_inliers=flags[hit].copy() if hit >= 0 else np.zeros(n, np.uint8),
               s=models[best, 0] if best >= 0 else f32(0), R=models[best, 1:10].reshape(3, 3) if best >= 0 else np.zeros((3, 3), f32),
               t=models[best, 10:13] if best >= 0 else np.zeros(3, f32),
               best_T12=out["T12"][best] if best >= 0 else np.zeros((4, 4), f32))
    return out


def sim3_iterations(n, probability, min_inliers, max_iterations):
    """SetRansacParameters (:114-138); 0 when n < min_inliers (iterate answers bNoMore without looking)"""
    if n < min_inliers:
        return 0
    eps = f32(f32(min_inliers) / f32(n))
    if min_inliers == n:
        k = 1
    else:
        den = math.log(1 - math.pow(float(eps), 3))
        q = math.log(1 - probability) / den if den != 0 else -math.inf
        k = max_iterations if not (q <= max_iterations - 1) else (1 if q < 1 else int(math.ceil(q)))
    return max(1, min(k, max_iterations))


def draw_sets(n, iterations, randint):
    """:163-177: per iteration 3 distinct indices < n without replacement - the drawn slot is overwritten by the last available
    index, which is dropped.  randint(lo, hi) is inclusive, as DUtils::Random::RandomInt."""
    sets = np.zeros((iterations, 3), np.int32)
    for it in range(iterations):
        avail = list(range(n))
        for j in range(3):
            k = randint(0, len(avail) - 1)
            sets[it, j] = avail[k]
            avail[k] = avail[-1]
            avail.pop()
    return sets


class Solver:
    """the sequential bookkeeping of Sim3Solver::iterate / find over a stored trace, chunked calls included"""

    def __init__(self, trace, min_inliers):
        self.tr, self.min_inliers = trace, min_inliers
        self.max_its, self.n = trace["iterations"], trace["n"]
        self.it, self.best_inliers, self.best = 0, 0, -1

    def iterate(self, k):
        """-> (T12 or None, no_more, inliers [n] uint8, n_inliers)"""
        inl = np.zeros(self.n, np.uint8)
        if self.max_its == 0:                     # N < mRansacMinInliers
            return None, True, inl, 0
        cur = 0
        while self.it < self.max_its and cur < k:
            cur += 1
            i = self.it
            self.it += 1
            c = int(self.tr["counts"][i])
            if c >= self.best_inliers:
                self.best_inliers, self.best = c, i
                if c > self.min_inliers:
                    return self.tr["T12"][i], False, self.tr["flags"][i].copy(), c
        return None, self.it >= self.max_its, inl, 0

    def find(self):
        return self.iterate(self.max_its)
