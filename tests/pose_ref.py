"""Optimizer::PoseOptimization (reference: src/Optimizer.cc:239-451) and the g2o pieces it drives, restated in numpy float64 with the
reference's float narrowings in the same places (DESIGN.md section 6 lists them).  Independent of the library: the GPU tests
compare k_pose_opt with this, the CPU tests check this against properties.

Sums over the edges run sequentially in a caller-given order (`order`, a permutation of the entry indices; default ascending), so
that the effect of the summation order can be measured.  Per round the trace records the iterations, the trials, which trials
were accepted, the smallest |rho| and the smallest |chi2 / threshold - 1| seen at the classification.
"""
import numpy as np

DBL_MAX = np.finfo(np.float64).max
DELTA_MONO = np.float64(np.float32(np.sqrt(5.991)))
DELTA_STEREO = np.float64(np.float32(np.sqrt(7.815)))
CHI2_MONO, CHI2_STEREO = np.float32(5.991), np.float32(7.815)

OBS_DTYPE = np.dtype([("valid", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4"),
                      ("wx", "<f4"), ("wy", "<f4"), ("wz", "<f4")])


def quat_from_R(R):
    """Eigen::Quaternion(Matrix3) -> x y z w"""
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


def normalize_rotation(q):
    if q[3] < 0.0:
        q = -q
    n = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
    return q / n


def quat_rotate(q, v):
    """Quaternion * Vector3; v is [3] or [3, n]"""
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


def se3_from_T(T):
    """Converter::toSE3Quat of the float 4x4 -> (t[3], q[4])"""
    T = np.asarray(T, np.float32).reshape(4, 4).astype(np.float64)
    return T[:3, 3].copy(), normalize_rotation(quat_from_R(T[:3, :3]))


def se3_to_T(t, q):
    T = np.eye(4)
    T[:3, :3] = quat_to_R(q)
    T[:3, 3] = t
    return T


def se3_oplus(t, q, x):
    """VertexSE3Expmap::oplusImpl: exp(x) * (t, q); x = omega | upsilon"""
    o0, o1, o2 = x[0], x[1], x[2]
    theta = np.sqrt((o0 * o0 + o1 * o1) + o2 * o2)
    Om = np.array([[0.0, -o2, o1], [o2, 0.0, -o0], [-o1, o0, 0.0]])
    Om2 = np.zeros((3, 3))
    for r in range(3):
        for c in range(3):
            Om2[r, c] = (Om[r, 0] * Om[0, c] + Om[r, 1] * Om[1, c]) + Om[r, 2] * Om[2, c]
    I = np.eye(3)
    if theta < 0.00001:
        R = (I + 1.0 * Om) + 1.0 * Om2
        V = R
    else:
        s, co = np.sin(theta), np.cos(theta)
        a = s / theta
        b = (1.0 - co) / (theta * theta)
        c2 = (theta - s) / (theta * theta * theta)
        R = (I + a * Om) + b * Om2
        V = (I + b * Om) + c2 * Om2
    qe = normalize_rotation(quat_from_R(R))
    te = np.array([(V[r, 0] * x[3] + V[r, 1] * x[4]) + V[r, 2] * x[5] for r in range(3)])
    rt = quat_rotate(qe, t)
    ax, ay, az, aw = qe
    bx, by, bz, bw = q
    qn = np.array([((aw * bx + ax * bw) + ay * bz) - az * by,
                   ((aw * by + ay * bw) + az * bx) - ax * bz,
                   ((aw * bz + az * bw) + ax * by) - ay * bx,
                   ((aw * bw - ax * bx) - ay * by) - az * bz])
    return te + rt, normalize_rotation(qn)


def _seqsum(a):
    """sequential (left to right) sum over axis 0; np.sum is pairwise"""
    if a.shape[0] == 0:
        return np.zeros(a.shape[1:])
    return np.cumsum(a, axis=0)[-1]


class Edges:
    """the valid entries of an observation array, widened to double, in summation order"""

    def __init__(self, obs, cam, order=None, exact_invz=False):
        obs = np.asarray(obs, OBS_DTYPE)
        idx = np.arange(len(obs)) if order is None else np.asarray(order)
        idx = idx[obs["valid"][idx] != 0]
        self.idx = idx
        self.exact_invz = exact_invz      # True: the stereo projection keeps 1 / z in double (a smooth cost, for the property tests)
        o = obs[idx]
        self.u, self.v, self.ur = (o[f].astype(np.float64) for f in ("u", "v", "ur"))
        self.mono = o["ur"] < 0
        self.is2 = o["inv_sigma2"].astype(np.float64)
        self.Xw = np.stack([o["wx"], o["wy"], o["wz"]]).astype(np.float64)
        self.fx, self.fy, self.cx, self.cy, self.bf = (np.float64(np.float32(c)) for c in cam[:5])
        self.delta = np.where(self.mono, DELTA_MONO, DELTA_STEREO)
        self.thr = np.where(self.mono, CHI2_MONO, CHI2_STEREO).astype(np.float32)

    def error(self, t, q):
        """-> (e[3, n], X[3, n]); a monocular edge is the stereo one with a zero third row"""
        X = quat_rotate(q, self.Xw) + t[:, None]
        x, y, z = X
        with np.errstate(all="ignore"):
            iz = 1.0 / z
            if not self.exact_invz:
                iz = iz.astype(np.float32).astype(np.float64)         # const float invz = 1.0f / trans_xyz[2]
            pu_s = (x * iz) * self.fx + self.cx
            e0 = np.where(self.mono, self.u - ((x / z) * self.fx + self.cx), self.u - pu_s)
            e1 = np.where(self.mono, self.v - ((y / z) * self.fy + self.cy), self.v - ((y * iz) * self.fy + self.cy))
            e2 = np.where(self.mono, 0.0, self.ur - (pu_s - self.bf * iz))
        return np.stack([e0, e1, e2]), X

    def chi2(self, e):
        oe = self.is2 * e
        return (e[0] * oe[0] + e[1] * oe[1]) + e[2] * oe[2]

    def huber(self, chi2, robust):
        """-> (rho0, rho1)"""
        rho0, w = chi2.copy(), np.ones_like(chi2)
        if robust:
            out = ~(chi2 <= self.delta * self.delta)
            with np.errstate(all="ignore"):
                s = np.sqrt(chi2)
                rho0 = np.where(out, (2.0 * s) * self.delta - self.delta * self.delta, rho0)
                w = np.where(out, self.delta / s, w)
        return rho0, w

    def jacobian(self, X):
        """-> J[3, 6, n]   (types_six_dof_expmap.cpp:266-288, :335-364)"""
        x, y, z = X
        fx, fy, bf = self.fx, self.fy, self.bf
        with np.errstate(all="ignore"):
            invz = 1.0 / z
        invz2 = invz * invz
        zero = np.zeros_like(x)
        J0 = [((x * y) * invz2) * fx, -(1.0 + ((x * x) * invz2)) * fx, (y * invz) * fx, -invz * fx, zero, (x * invz2) * fx]
        J1 = [(1.0 + (y * y) * invz2) * fy, ((-x * y) * invz2) * fy, (-x * invz) * fy, zero, -invz * fy, (y * invz2) * fy]
        J2 = [J0[0] - (bf * y) * invz2, J0[1] + (bf * x) * invz2, J0[2], J0[3], zero, J0[5] - bf * invz2]
        J2 = [np.where(self.mono, 0.0, j) for j in J2]
        return np.array([J0, J1, J2])

    def linearize(self, t, q, act, robust):
        """one pass at (t, q) over the active edges -> (H[6, 6], b[6], sum rho0, chi2[n])"""
        e, X = self.error(t, q)
        chi2 = self.chi2(e)
        rho0, w = self.huber(chi2, robust)
        J = self.jacobian(X)
        oe = self.is2 * e
        wo = w * self.is2
        H = np.zeros((6, 6))
        for j in range(6):
            for l in range(j, 6):
                term = ((J[0, j] * wo) * J[0, l] + (J[1, j] * wo) * J[1, l]) + (J[2, j] * wo) * J[2, l]
                H[j, l] = H[l, j] = _seqsum(term[act])
        b = np.zeros(6)
        for j in range(6):
            term = w * ((J[0, j] * oe[0] + J[1, j] * oe[1]) + J[2, j] * oe[2])
            b[j] = -_seqsum(term[act])       # b -= term, edge after edge, from 0: the negated sum bit for bit
        return H, b, _seqsum(rho0[act]), chi2

    def robust_chi2(self, t, q, act, robust):
        e, _ = self.error(t, q)
        chi2 = self.chi2(e)
        rho0, _ = self.huber(chi2, robust)
        return _seqsum(rho0[act]), chi2


def solve6(H, b, lam):
    """(H + lam I) x = b by an unpivoted LDL^T -> (ok, x); x = 0 when a pivot is not positive"""
    A = H.copy()
    for j in range(6):
        A[j, j] += lam
    L = np.zeros((6, 6))
    D = np.zeros(6)
    ok = True
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j, j]
            for m in range(j):
                d -= (L[j, m] * L[j, m]) * D[m]
            if not (d > 0.0) or not (d <= DBL_MAX):
                ok = False
            D[j] = d
            for i in range(j + 1, 6):
                s = A[i, j]
                for m in range(j):
                    s -= (L[i, m] * L[j, m]) * D[m]
                L[i, j] = s / d
        y = np.zeros(6)
        for i in range(6):
            s = b[i]
            for m in range(i):
                s -= L[i, m] * y[m]
            y[i] = s
        y = y / D
        x = np.zeros(6)
        for i in range(5, -1, -1):
            s = y[i]
            for m in range(i + 1, 6):
                s -= L[m, i] * x[m]
            x[i] = s
    if not ok:
        x = np.zeros(6)
    return ok, x


def pose_optimization(obs, cam, Tcw, outlier=None, order=None, edges=None):
    """-> dict(Tcw float32 [4, 4], outlier uint8 [n], ngood, correspondences, bad, rounds, iterations[4], trials[4], t, q, trace)
    cam = (fx, fy, cx, cy, bf, ...).  trace[r] = dict(iterations, trials, accepted [bool per trial], min_abs_rho, min_margin,
    margins / flags [per valid entry, in summation order], t, q)."""
    obs = np.asarray(obs, OBS_DTYPE)
    n = len(obs)
    out = np.zeros(n, np.uint8) if outlier is None else np.asarray(outlier, np.uint8).copy()
    E = Edges(obs, cam, order) if edges is None else edges     # edges: a prebuilt set (a test may give it exact double observations)
    out[E.idx] = 0
    nInit = len(E.idx)
    Tin = np.asarray(Tcw, np.float32).reshape(4, 4)
    t0, q0 = se3_from_T(Tin)
    res = dict(Tcw=Tin.copy(), outlier=out, ngood=0, correspondences=nInit, bad=0, rounds=0, iterations=[0] * 4, trials=[0] * 4,
               t=t0, q=q0, trace=[])
    if nInit < 3:
        return res
    flagged = np.zeros(nInit, bool)
    t, q = t0, q0
    nBad = 0
    for rnd in range(4):
        t, q = t0.copy(), q0.copy()
        act = ~flagged
        robust = rnd <= 2
        last = np.zeros(nInit)
        lam, ni, nbad_it = 0.0, 2.0, 0
        tr = dict(iterations=0, trials=0, accepted=[], min_abs_rho=np.inf)
        with np.errstate(all="ignore"):
            for it in range(10):
                H, b, cur, c2 = E.linearize(t, q, act, robust)
                last[act] = c2[act]
                ini = cur
                if it == 0:
                    lam, ni, nbad_it = 1e-5 * max(0.0, *[abs(H[j, j]) for j in range(6)]), 2.0, 0
                rho, qn = 0.0, 0
                for trial in range(10):
                    bt, bq = t, q
                    ok, x = solve6(H, b, lam)
                    if ok:
                        t, q = se3_oplus(t, q, x)
                    tmp, c2 = E.robust_chi2(t, q, act, robust)
                    last[act] = c2[act]
                    if not ok:
                        tmp = DBL_MAX
                    scale = 0.0
                    for j in range(6):
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
                        t, q = bt, bq
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
            # classification: an active edge keeps the chi2 of its last evaluation, a flagged one is evaluated at the round's pose
            e, _ = E.error(t, q)
            c2 = np.where(flagged, E.chi2(e), last).astype(np.float32)
            flagged = c2 > E.thr
            margins = np.abs(c2.astype(np.float64) / E.thr.astype(np.float64) - 1.0)
        nBad = int(flagged.sum())
        tr.update(min_margin=float(margins.min()), margins=margins, t=t.copy(), q=q.copy(), flags=flagged.copy())
        res["trace"].append(tr)
        res["iterations"][rnd], res["trials"][rnd] = tr["iterations"], tr["trials"]
        res["rounds"] = rnd + 1
        if nInit < 10:
            break
    out[E.idx] = flagged
    res.update(Tcw=se3_to_T(t, q).astype(np.float32), ngood=nInit - nBad, bad=nBad, t=t, q=q)
    return res
