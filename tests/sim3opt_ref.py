"""Optimizer::OptimizeSim3 (reference: src/Optimizer.cc:1051-1246) and the g2o pieces it drives - VertexSim3Expmap, Sim3(Vector7d),
EdgeSim3ProjectXYZ / EdgeInverseSim3ProjectXYZ, BaseBinaryEdge's numeric linearizeOplus (central differences, delta = 1e-9), the
Huber kernel, the Levenberg-Marquardt schedule - restated in numpy float64 with the reference's float narrowings in the same places
(k_sim3_opt).  Independent of the library: the GPU tests compare k_sim3_opt with this, the CPU tests check this
against properties and the kernel's text, compiled for the host, against this byte for byte.

The estimate is a scalar state (q = x y z w, t, s); everything per edge is a vector over the matches.  Sums over the matches run
sequentially in a caller-given order (`order`, a permutation of the rows; default ascending), edge 12 of a match before its edge 21.
`perturb` (a numpy Generator): every result of exp / sin / cos is moved by up to +-ULPS units in the last place, which models a
math library other than this host's.  ULPS = 2 is ASSUMED: no statement of the device library's double-precision error bounds is
installed with the toolchain on the build machine, so it was not looked up.
Per round the trace records iterations, trials, which trials were accepted, the smallest |rho|, and at the classification the
smallest |chi2 / th2 - 1| over the live edges.
"""
import math

import numpy as np

DBL_MAX = np.finfo(np.float64).max
DELTA = 1e-9
SCALAR = 1.0 / (2 * 1e-9)
ULPS = 2

MATCH_DTYPE = np.dtype([("w1", "<f4", (3,)), ("w2", "<f4", (3,)), ("u1", "<f4"), ("v1", "<f4"), ("u2", "<f4"), ("v2", "<f4"),
                        ("inv_sigma2_1", "<f4"), ("inv_sigma2_2", "<f4")])
PROBLEM_DTYPE = np.dtype([("Tcw1", "<f4", (16,)), ("Tcw2", "<f4", (16,)), ("K1", "<f4", (4,)), ("K2", "<f4", (4,)), ("s", "<f4"),
                          ("R", "<f4", (9,)), ("t", "<f4", (3,)), ("th2", "<f4"), ("fix_scale", "<i4")])


class Lib:
    """exp / sin / cos of this host's libm (the one the lockstep program links), optionally moved by up to +-ULPS ulp"""

    def __init__(self, rng=None):
        self.rng = rng

    def _f(self, fn, x):
        try:
            v = fn(float(x))
        except OverflowError:
            v = math.inf
        except ValueError:
            v = math.nan
        if self.rng is not None and math.isfinite(v):
            v = v + int(self.rng.integers(-ULPS, ULPS + 1)) * float(np.spacing(abs(v)))
        return np.float64(v)

    def exp(self, x):
        return self._f(math.exp, x)

    def sin(self, x):
        return self._f(math.sin, x)

    def cos(self, x):
        return self._f(math.cos, x)


def quat_from_R(R):
    """Eigen::Quaternion(Matrix3) -> x y z w, not normalised"""
    q = np.zeros(4)
    t = R[0, 0] + R[1, 1] + R[2, 2]
    if t > 0.0:
        t = np.sqrt(t + 1.0)
        q[3] = 0.5 * t
        t = 0.5 / t
        q[0] = (R[2, 1] - R[1, 2]) * t
        q[1] = (R[0, 2] - R[2, 0]) * t
        q[2] = (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def quat_rotate(q, v):
    """Quaternion * Vector3 (_transformVector); v is [3] or [3, n]"""
    uv0 = q[1] * v[2] - q[2] * v[1]
    uv1 = q[2] * v[0] - q[0] * v[2]
    uv2 = q[0] * v[1] - q[1] * v[0]
    uv0 = uv0 + uv0
    uv1 = uv1 + uv1
    uv2 = uv2 + uv2
    return np.array([(v[0] + q[3] * uv0) + (q[1] * uv2 - q[2] * uv1),
                     (v[1] + q[3] * uv1) + (q[2] * uv0 - q[0] * uv2),
                     (v[2] + q[3] * uv2) + (q[0] * uv1 - q[1] * uv0)])


def quat_to_R(q):
    tx, ty, tz = 2.0 * q[0], 2.0 * q[1], 2.0 * q[2]
    twx, twy, twz = tx * q[3], ty * q[3], tz * q[3]
    txx, txy, txz = tx * q[0], ty * q[0], tz * q[0]
    tyy, tyz, tzz = ty * q[1], tz * q[1], tz * q[2]
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


class Sim3:
    """g2o::Sim3: q (x y z w), t, s"""

    def __init__(self, q, t, s):
        self.q, self.t, self.s = np.asarray(q, np.float64), np.asarray(t, np.float64), np.float64(s)

    @staticmethod
    def from_Rts(R, t, s):
        """Sim3(Matrix3d, Vector3d, double) of the solver's floats, widened"""
        R = np.asarray(R, np.float32).reshape(3, 3).astype(np.float64)
        return Sim3(quat_from_R(R), np.asarray(t, np.float32).astype(np.float64), np.float64(np.float32(s)))

    def __mul__(a, b):      # noqa: N805   sim3.h:266-272, no normalisation
        ax, ay, az, aw = a.q
        bx, by, bz, bw = b.q
        q = np.array([((aw * bx + ax * bw) + ay * bz) - az * by,
                      ((aw * by + ay * bw) + az * bx) - ax * bz,
                      ((aw * bz + az * bw) + ax * by) - ay * bx,
                      ((aw * bw - ax * bx) - ay * by) - az * bz])
        return Sim3(q, a.s * quat_rotate(a.q, b.t) + a.t, a.s * b.s)

    def inverse(self):      # sim3.h:233-236
        qc = np.array([-self.q[0], -self.q[1], -self.q[2], self.q[3]])
        k = -1. / self.s
        return Sim3(qc, quat_rotate(qc, k * self.t), 1. / self.s)

    def map(self, P):       # s * (r * xyz) + t; P [3] or [3, n]
        r = quat_rotate(self.q, P)
        t = self.t if r.ndim == 1 else self.t[:, None]
        return self.s * r + t

    def matrix(self):
        """Converter::toCvMat(g2o::Sim3): s * R | t, float 4x4"""
        T = np.eye(4)
        T[:3, :3] = self.s * quat_to_R(self.q)
        T[:3, 3] = self.t
        return T.astype(np.float32)

    def vec(self):
        return np.concatenate([self.q, self.t, [self.s]])


def sim3_exp(u, lib):
    """Sim3(const Vector7d &) (sim3.h:70-142): u = omega | upsilon | sigma, the four branches as written"""
    o0, o1, o2, sigma = u[0], u[1], u[2], u[6]
    theta = np.sqrt((o0 * o0 + o1 * o1) + o2 * o2)
    Om = np.array([[0.0, -o2, o1], [o2, 0.0, -o0], [-o1, o0, 0.0]])
    Om2 = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            Om2[r, c] = (Om[r, 0] * Om[0, c] + Om[r, 1] * Om[1, c]) + Om[r, 2] * Om[2, c]
    s = lib.exp(sigma)
    eps = 0.00001
    if abs(sigma) < eps:
        C = 1.0
        if theta < eps:
            A, B, ra, rb = 1. / 2., 1. / 6., 1.0, 1.0
        else:
            theta2, si, co = theta * theta, lib.sin(theta), lib.cos(theta)
            A = (1.0 - co) / theta2
            B = (theta - si) / (theta2 * theta)
            ra, rb = si / theta, (1.0 - co) / (theta * theta)
    else:
        C = (s - 1.0) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - 1.0) * s + 1.0) / sigma2
            B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma)
            ra, rb = 1.0, 1.0
        else:
            si, co = lib.sin(theta), lib.cos(theta)
            ra, rb = si / theta, (1.0 - co) / (theta * theta)
            a, b, theta2, sigma2 = s * si, s * co, theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (1.0 - b) * theta) / (theta * c)
            B = ((C - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2
    I = np.eye(3)
    R = (I + ra * Om) + rb * Om2
    W = (A * Om + B * Om2) + C * I
    t = np.array([(W[r, 0] * u[3] + W[r, 1] * u[4]) + W[r, 2] * u[5] for r in range(3)])
    return Sim3(quat_from_R(R), t, s)


def _seqsum(a):
    """sequential (left to right) sum over axis 0; np.sum is pairwise"""
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:])
    return np.cumsum(a, axis=0)[-1]


def transform(T, X):
    """R*P+t of a cv::Mat expression on CV_32F: products in double, left to right, + t in double, narrowed once.  X [n, 3] float32"""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    X = np.asarray(X, np.float32).astype(np.float64)
    return np.stack([((T[k, 0] * X[:, 0] + T[k, 1] * X[:, 1]) + T[k, 2] * X[:, 2]) + T[k, 3] for k in range(3)]).astype(np.float32)


class Edges:
    """the matches of a problem, widened to double, in summation order: side 0 = edge 12 (point 2 through S into camera 1),
    side 1 = edge 21 (point 1 through S^-1 into camera 2)"""

    def __init__(self, matches, prob, order=None):
        m = np.asarray(matches, MATCH_DTYPE)
        self.idx = np.arange(len(m)) if order is None else np.asarray(order)
        m = m[self.idx]
        P1 = transform(prob["Tcw1"], m["w1"].reshape(-1, 3)).astype(np.float64)
        P2 = transform(prob["Tcw2"], m["w2"].reshape(-1, 3)).astype(np.float64)
        self.P = [P2, P1]
        self.uv = [np.stack([m["u1"], m["v1"]]).astype(np.float64), np.stack([m["u2"], m["v2"]]).astype(np.float64)]
        self.is2 = [m["inv_sigma2_1"].astype(np.float64), m["inv_sigma2_2"].astype(np.float64)]
        self.K = [np.asarray(prob["K1"], np.float32).astype(np.float64), np.asarray(prob["K2"], np.float32).astype(np.float64)]
        self.th2 = np.float64(np.float32(prob["th2"]))
        self.delta = np.float64(np.float32(np.sqrt(np.float64(np.float32(prob["th2"])))))

    def error(self, side, S):
        """obs - cam_map(project(S.map(P))) -> e [2, n]; S is the estimate for side 0, its inverse for side 1"""
        x, y, z = S.map(self.P[side])
        fx, fy, cx, cy = self.K[side]
        u, v = self.uv[side]
        return np.stack([u - ((x / z) * fx + cx), v - ((y / z) * fy + cy)])

    def chi2(self, side, e):
        oe = self.is2[side] * e
        return e[0] * oe[0] + e[1] * oe[1]

    def huber(self, chi2):
        dsqr = self.delta * self.delta
        out = ~(chi2 <= dsqr)
        s = np.sqrt(chi2)
        return np.where(out, (2.0 * s) * self.delta - dsqr, chi2), np.where(out, self.delta / s, 1.0)

    def jacobian(self, side, pert):
        """the numeric Jacobian (base_binary_edge.hpp:147-198) at the 14 perturbed estimates -> J [2, 7, n]"""
        n = self.P[side].shape[1]
        J = np.zeros((2, 7, n))
        for d in range(7):
            J[:, d] = SCALAR * (self.error(side, pert[2 * d]) - self.error(side, pert[2 * d + 1]))
        return J

    def evaluate(self, S, act):
        """a trial's pass -> (sum rho0 over the active matches, chi2 [2, n])"""
        Ss = [S, S.inverse()]
        c2 = np.stack([self.chi2(sd, self.error(sd, Ss[sd])) for sd in range(2)])
        rho0 = np.stack([self.huber(c2[sd])[0] for sd in range(2)])
        return _seqsum(rho0.T[act].reshape(-1)), c2            # match after match, edge 12 before edge 21

    def linearize(self, S, act, fix_scale, lib):
        """one linearisation at S over the active matches -> (H [7, 7], b [7], sum rho0, chi2 [2, n], J)"""
        pert = []
        for k in range(14):
            upd = np.zeros(7)
            upd[k >> 1] = -DELTA if k & 1 else DELTA
            if fix_scale:
                upd[6] = 0.0
            pert.append(sim3_exp(upd, lib) * S)
        perts = [pert, [p.inverse() for p in pert]]
        Ss = [S, S.inverse()]
        e = [self.error(sd, Ss[sd]) for sd in range(2)]
        c2 = np.stack([self.chi2(sd, e[sd]) for sd in range(2)])
        hub = [self.huber(c2[sd]) for sd in range(2)]
        J = [self.jacobian(sd, perts[sd]) for sd in range(2)]
        H = np.zeros((7, 7))
        b = np.zeros(7)

        def both(t0, t1):       # [n] per side -> the active matches' terms interleaved 12, 21, 12, 21, ...
            return np.stack([t0, t1]).T[act].reshape(-1)
        wo = [hub[sd][1] * self.is2[sd] for sd in range(2)]
        oe = [self.is2[sd] * e[sd] for sd in range(2)]
        for j in range(7):
            for l in range(j, 7):
                term = [(J[sd][0, j] * wo[sd]) * J[sd][0, l] + (J[sd][1, j] * wo[sd]) * J[sd][1, l] for sd in range(2)]
                H[j, l] = H[l, j] = _seqsum(both(*term))
            term = [hub[sd][1] * (J[sd][0, j] * oe[sd][0] + J[sd][1, j] * oe[sd][1]) for sd in range(2)]
            b[j] = -_seqsum(both(*term))         # b -= term, edge after edge, from 0: the negated sum bit for bit
        return H, b, _seqsum(both(hub[0][0], hub[1][0])), c2, J


def solve7(H, b, lam):
    """(H + lam I) x = b by an unpivoted LDL^T -> (ok, x); x = 0 when a pivot is not positive"""
    N = 7
    A = H.copy()
    for j in range(N):
        A[j, j] += lam
    L = np.zeros((N, N))
    D = np.zeros(N)
    ok = True
    for j in range(N):
        d = A[j, j]
        for m in range(j):
            d -= (L[j, m] * L[j, m]) * D[m]
        if not (d > 0.0) or not (d <= DBL_MAX):
            ok = False
        D[j] = d
        for i in range(j + 1, N):
            s = A[i, j]
            for m in range(j):
                s -= (L[i, m] * L[j, m]) * D[m]
            L[i, j] = s / d
    y = np.zeros(N)
    for i in range(N):
        s = b[i]
        for m in range(i):
            s -= L[i, m] * y[m]
        y[i] = s
    y = y / D
    x = np.zeros(N)
    for i in range(N - 1, -1, -1):
        s = y[i]
        for m in range(i + 1, N):
            s -= L[m, i] * x[m]
        x[i] = s
    if not ok:
        x = np.zeros(N)
    return ok, x


def optimize_sim3(matches, prob, order=None, perturb=None):
    """-> dict(S12 float32 [4, 4], dropped uint8 [n], ninliers, correspondences, bad, rounds, iterations[2], trials[2], q, t, s,
    sim3 (the Sim3), trace).  trace[r] = dict(iterations, trials, accepted, min_abs_rho, min_margin, margins [2, live], flags)"""
    matches = np.asarray(matches, MATCH_DTYPE)
    n = len(matches)
    lib = Lib(perturb)
    E = Edges(matches, prob, order)
    fix = int(prob["fix_scale"]) != 0
    S0 = Sim3.from_Rts(prob["R"], prob["t"], prob["s"])
    S = S0
    dropped = np.zeros(n, bool)          # in summation order
    res = dict(correspondences=n, bad=0, rounds=0, iterations=[0, 0], trials=[0, 0], trace=[], ninliers=0)
    nBad, done = 0, False
    with np.errstate(all="ignore"):
        for rnd in range(2 if n >= 1 else 0):
            maxit = 5 if rnd == 0 else (10 if nBad > 0 else 5)
            act = ~dropped
            over = np.zeros(n, bool)
            lam, ni, nbad_it = 0.0, 2.0, 0
            tr = dict(iterations=0, trials=0, accepted=[], min_abs_rho=np.inf)
            last = np.zeros((2, n))
            for it in range(maxit):
                H, b, cur, c2, _ = E.linearize(S, act, fix, lib)
                last = c2
                ini = cur
                if it == 0:
                    lam, ni, nbad_it = 1e-5 * max(0.0, *[abs(H[j, j]) for j in range(7)]), 2.0, 0
                rho, qn = 0.0, 0
                for trial in range(10):
                    backup = S
                    ok, x = solve7(H, b, lam)
                    if fix:
                        x[6] = 0.0
                    if ok:
                        S = sim3_exp(x, lib) * S
                    tmp, c2 = E.evaluate(S, act)
                    last = c2
                    if not ok:
                        tmp = DBL_MAX
                    scale = 0.0
                    for j in range(7):
                        scale += x[j] * (lam * x[j] + b[j])
                    scale += 1e-3
                    rho = (cur - tmp) / scale
                    tr["min_abs_rho"] = min(tr["min_abs_rho"], abs(rho)) if rho == rho else 0.0
                    if rho > 0.0 and abs(tmp) <= DBL_MAX:
                        u = 2.0 * rho - 1.0
                        alpha = min(1.0 - (u * u) * u, 2.0 / 3.0)
                        lam *= max(1.0 / 3.0, alpha)
                        ni = 2.0
                        cur = tmp
                        tr["accepted"].append(True)
                    else:
                        lam *= ni
                        ni *= 2.0
                        S = backup
                        tr["accepted"].append(False)
                    qn += 1
                    if not (rho < 0.0):
                        break
                tr["iterations"] += 1
                tr["trials"] += qn
                if qn == 10 or rho == 0.0:
                    break
                nbad_it = nbad_it + 1 if (ini - cur) * 1e3 < ini else 0
                if nbad_it >= 3:
                    break
            # classification on the edges' last evaluation: a live match is dropped if either edge exceeds th2
            over = act & ((last[0] > E.th2) | (last[1] > E.th2))
            margins = np.abs(last[:, act] / E.th2 - 1.0)
            dropped = dropped | over
            nBad = int(dropped.sum())
            tr.update(min_margin=float(margins.min()) if margins.size else np.inf, margins=margins, flags=dropped.copy(), sim3=S)
            res["trace"].append(tr)
            res["iterations"][rnd], res["trials"][rnd] = tr["iterations"], tr["trials"]
            res["rounds"] = rnd + 1
            if rnd == 1:
                done = True
            if n - nBad < 10:
                break
    So = S if done else S0
    out = np.zeros(n, np.uint8)
    out[E.idx] = dropped
    res.update(S12=So.matrix(), dropped=out, ninliers=(n - nBad) if done else 0, bad=nBad, q=So.q.copy(), t=So.t.copy(), s=So.s,
               sim3=So, start=S0)
    return res
