"""Optimizer::LocalBundleAdjustment (reference: src/Optimizer.cc:453-780), Optimizer::BundleAdjustment (:49-237) and the g2o pieces
they drive (types_six_dof_expmap, base_binary_edge.hpp, block_solver.hpp, optimization_algorithm_levenberg, sparse_optimizer),
restated in numpy float64 with the reference's float narrowings in the same places ("k_lba_*").  Independent
of the library: the GPU tests compare the kernels of csrc/orbx_lba.hip with this, the CPU tests check this against properties
and demand the kernels' text, run as one thread per workgroup, to give the same bytes.

Every sum has an owner and runs sequentially over the owner's terms in ascending `key` (the input index of an observation, the
index of a point); a caller may give a random generator instead (`order`), which draws the keys, so that the effect of the
summation order can be measured; `perturb` moves every sin / cos by up to +-2 ulp."""
import numpy as np

from pose_ref import DBL_MAX, normalize_rotation, quat_from_R, quat_rotate, quat_to_R

KF_DTYPE = np.dtype([("Tcw", "<f4", (16,)), ("fx", "<f4"), ("fy", "<f4"), ("cx", "<f4"), ("cy", "<f4"), ("bf", "<f4"), ("fixed", "<i4")])
PT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4")])
OBS_DTYPE = np.dtype([("kf", "<i4"), ("pt", "<i4"), ("u", "<f4"), ("v", "<f4"), ("ur", "<f4"), ("inv_sigma2", "<f4")])
STOP_BEFORE, STOP_ROUND1, STOP_BETWEEN, STOP_ROUND2 = 1, 2, 3, 4
CHI2_MONO, CHI2_STEREO = 5.991, 7.815
MAX_TRIALS = 10


def schedule_local():
    """:569-570, :655-707"""
    return dict(rounds=2, iterations=[5, 10], robust=[1, 0], delta_mono=np.float32(np.sqrt(5.991)), delta_stereo=np.float32(np.sqrt(7.815)),
                classify=1, check_stop_first=1)


def schedule_global(iterations, robust):
    """:85-86, :187-188"""
    return dict(rounds=1, iterations=[iterations, 0], robust=[int(bool(robust)), 0], delta_mono=np.float32(np.sqrt(5.99)),
                delta_stereo=np.float32(np.sqrt(7.815)), classify=0, check_stop_first=0)


def se3_oplus(T, x, perturb=None):
    """VertexSE3Expmap::oplusImpl: exp(x) * T; T = t[3] | q[4], x = omega | upsilon (tests/pose_ref.py's, with the perturbation)"""
    t, q = T[:3], T[3:]
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
        if perturb is not None:
            s = s + perturb.integers(-2, 3) * np.spacing(s)
            co = co + perturb.integers(-2, 3) * np.spacing(co)
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
    return np.concatenate([te + rt, normalize_rotation(qn)])


def quat_from_true(T):
    """the unit quaternion (x y z w, w >= 0) of a 4x4 pose"""
    return normalize_rotation(quat_from_R(np.asarray(T, np.float64)[:3, :3]))


class OwnerSum:
    """sequential sums of terms by owner, an owner's terms in ascending key: acc = init; acc -+= term, term after term"""

    def __init__(self, owner, key, nown):
        owner = np.asarray(owner, np.int64)
        idx = np.lexsort((key, owner))
        o = owner[idx]
        start = np.searchsorted(o, np.arange(nown))
        rank = np.arange(len(o)) - start[o] if len(o) else np.zeros(0, np.int64)
        self.nown = nown
        self.groups = [(idx[rank == r], o[rank == r]) for r in range(int(rank.max()) + 1)] if len(o) else []

    def __call__(self, terms, init=None, sign=1):
        acc = np.zeros((self.nown,) + terms.shape[1:]) if init is None else init.copy()
        for ii, oo in self.groups:
            if sign > 0:
                acc[oo] += terms[ii]
            else:
                acc[oo] -= terms[ii]
        return acc


def _seqsum(a, perm=None):
    if len(a) == 0:
        return 0.0
    return float(np.cumsum(a if perm is None else a[perm])[-1])


class Problem:
    """the arrays of one call, widened as the reference widens them"""

    def __init__(self, kfs, pts, obs, exact_invz=False):
        self.kfs, self.ptsf, self.obs = np.asarray(kfs, KF_DTYPE), np.asarray(pts, PT_DTYPE), np.asarray(obs, OBS_DTYPE)
        self.K, self.P, self.E = len(self.kfs), len(self.ptsf), len(self.obs)
        self.exact_invz = exact_invz      # True: the stereo projection keeps 1 / z and bf / z in double (a smooth cost, for the property tests)
        o, k = self.obs, self.kfs
        self.ekf, self.ept = o["kf"].astype(np.int64), o["pt"].astype(np.int64)
        self.u, self.v, self.ur, self.is2 = (o[f].astype(np.float64) for f in ("u", "v", "ur", "inv_sigma2"))
        self.mono = o["ur"] < 0
        self.fx, self.fy, self.cx, self.cy, self.bf = (k[f][self.ekf].astype(np.float64) for f in ("fx", "fy", "cx", "cy", "bf"))
        self.bff = k["bf"][self.ekf].astype(np.float32)
        self.fixed = k["fixed"] != 0
        self.thr = np.where(self.mono, CHI2_MONO, CHI2_STEREO)

    def initial(self):
        """-> (poses [K, 7] t | q of Converter::toSE3Quat, points [P, 3])"""
        poses = np.zeros((self.K, 7))
        for i in range(self.K):
            T = self.kfs["Tcw"][i].reshape(4, 4).astype(np.float64)
            poses[i, :3] = T[:3, 3]
            poses[i, 3:] = normalize_rotation(quat_from_R(T[:3, :3]))
        pts = np.stack([self.ptsf["x"], self.ptsf["y"], self.ptsf["z"]], 1).astype(np.float64).reshape(self.P, 3)
        return poses, pts

    def camera_points(self, poses, pts):
        T = poses[self.ekf].T                   # [7, E]
        X = quat_rotate(T[3:], pts[self.ept].T)
        return X[0] + T[0], X[1] + T[1], X[2] + T[2], T[3:]

    def evaluate(self, poses, pts, robust, dMono, dStereo, lin):
        """every edge at (poses, pts) -> dict(chi2, rho0, z, and with lin: ed [E, 54] = Hll 6 | bl 3 | Hpp 21 | bp 6 | W 18)"""
        x, y, z, q = self.camera_points(poses, pts)
        fx, fy, cx, cy, bf, mono = self.fx, self.fy, self.cx, self.cy, self.bf, self.mono
        with np.errstate(all="ignore"):
            iz = 1.0 / z
            if self.exact_invz:
                bfiz = bf * iz
            else:
                izf = iz.astype(np.float32)                               # const float invz = 1.0f / trans_xyz[2]
                iz = izf.astype(np.float64)
                bfiz = (self.bff * izf).astype(np.float64)                # const float &bf: a float product
            pu = (x * iz) * fx + cx
            e0 = np.where(mono, self.u - ((x / z) * fx + cx), self.u - pu)
            e1 = np.where(mono, self.v - ((y / z) * fy + cy), self.v - ((y * iz) * fy + cy))
            e2 = np.where(mono, 0.0, self.ur - (pu - bfiz))
            is2 = self.is2
            oe0, oe1, oe2 = is2 * e0, is2 * e1, is2 * e2
            chi2 = (e0 * oe0 + e1 * oe1) + e2 * oe2
            delta = np.where(mono, np.float64(dMono), np.float64(dStereo))
            dsqr = delta * delta
            rho0, w = chi2.copy(), np.ones_like(chi2)
            if robust:
                out = ~(chi2 <= dsqr)
                s = np.sqrt(chi2)
                rho0 = np.where(out, (2.0 * s) * delta - dsqr, rho0)
                w = np.where(out, delta / s, w)
            res = dict(chi2=chi2, rho0=rho0, z=z, e=np.stack([e0, e1, e2]))
            if not lin:
                return res
            R = quat_to_R(q)                                              # [3, 3, E]
            z_2 = z * z
            s = -1. / z
            zero = np.zeros_like(z)
            t0 = [s * fx, s * zero, s * (((-x) / z) * fx)]
            t1 = [s * zero, s * fy, s * (((-y) / z) * fy)]
            A = np.zeros((3, 3, self.E))
            for k in range(3):
                a0m = (t0[0] * R[0, k] + t0[1] * R[1, k]) + t0[2] * R[2, k]
                a1m = (t1[0] * R[0, k] + t1[1] * R[1, k]) + t1[2] * R[2, k]
                a0s = ((-fx) * R[0, k]) / z + ((fx * x) * R[2, k]) / z_2
                a1s = ((-fy) * R[1, k]) / z + ((fy * y) * R[2, k]) / z_2
                a2s = a0s - (bf * R[2, k]) / z_2
                A[0, k], A[1, k], A[2, k] = np.where(mono, a0m, a0s), np.where(mono, a1m, a1s), np.where(mono, 0.0, a2s)
            B = np.zeros((3, 6, self.E))
            B[0, 0] = ((x * y) / z_2) * fx
            B[0, 1] = -(1 + ((x * x) / z_2)) * fx
            B[0, 2] = (y / z) * fx
            B[0, 3] = (-1. / z) * fx
            B[0, 5] = (x / z_2) * fx
            B[1, 0] = (1 + (y * y) / z_2) * fy
            B[1, 1] = (((-x) * y) / z_2) * fy
            B[1, 2] = ((-x) / z) * fy
            B[1, 4] = (-1. / z) * fy
            B[1, 5] = (y / z_2) * fy
            B[2, 0] = np.where(mono, 0.0, B[0, 0] - (bf * y) / z_2)
            B[2, 1] = np.where(mono, 0.0, B[0, 1] + (bf * x) / z_2)
            B[2, 2] = np.where(mono, 0.0, B[0, 2])
            B[2, 3] = np.where(mono, 0.0, B[0, 3])
            B[2, 5] = np.where(mono, 0.0, B[0, 5] - bf / z_2)
            wo = w * is2
            ed = []
            for j in range(3):
                for l in range(j, 3):
                    ed.append(((A[0, j] * wo) * A[0, l] + (A[1, j] * wo) * A[1, l]) + (A[2, j] * wo) * A[2, l])
            for j in range(3):
                ed.append(-(w * ((A[0, j] * oe0 + A[1, j] * oe1) + A[2, j] * oe2)))
            for j in range(6):
                for l in range(j, 6):
                    ed.append(((B[0, j] * wo) * B[0, l] + (B[1, j] * wo) * B[1, l]) + (B[2, j] * wo) * B[2, l])
            for j in range(6):
                ed.append(-(w * ((B[0, j] * oe0 + B[1, j] * oe1) + B[2, j] * oe2)))
            for j in range(6):
                for l in range(3):
                    ed.append(((B[0, j] * wo) * A[0, l] + (B[1, j] * wo) * A[1, l]) + (B[2, j] * wo) * A[2, l])
            res.update(ed=np.stack(ed, 1), A=A, B=B, w=w)
        return res


UP6 = [(j, l) for j in range(6) for l in range(j, 6)]      # the 21 upper entries of Hpp, row-major
DIAG6, DIAG3 = [0, 6, 11, 15, 18, 20], [0, 3, 5]


class Round:
    """initializeOptimization(0) for the edges in `active`: the columns of the free poses that still have an edge, the points that
    do, and the owners' sums"""

    def __init__(self, pb, active, order=None):
        self.pb, self.active = pb, active
        E, K, P = pb.E, pb.K, pb.P
        has = np.zeros(K, bool)
        has[pb.ekf[active]] = True
        free = has & ~pb.fixed
        self.col = np.where(free, np.cumsum(free) - 1, -1)
        self.nf = int(free.sum())
        self.kf_of_col = np.nonzero(free)[0]
        self.pact = np.zeros(P, bool)
        self.pact[pb.ept[active]] = True
        rnd = (lambda n: np.arange(n)) if order is None else (lambda n: order.random(n))
        ae = np.nonzero(active)[0]
        self.ae = ae
        self.sum_pt = OwnerSum(pb.ept[ae], rnd(E)[ae], P)
        ecol = self.col[pb.ekf]
        pe = ae[ecol[ae] >= 0]                                  # active edges of a column
        self.pe = pe
        self.sum_pose = OwnerSum(ecol[pe], rnd(E)[pe], self.nf)
        self.sum_back = OwnerSum(pb.ept[pe], rnd(E)[pe], P)
        # the Schur terms: per point every ordered pair (ea, eb) of its column edges with col(ea) <= col(eb)
        ea, eb = [], []
        spe = pe[np.lexsort((ecol[pe], pb.ept[pe]))]            # by point, then by column
        bounds = np.searchsorted(pb.ept[spe], np.arange(P + 1))
        for p in range(P):
            el = spe[bounds[p]:bounds[p + 1]]
            if len(el):
                i1, i2 = np.triu_indices(len(el))
                ea.append(el[i1]); eb.append(el[i2])
        ea = np.concatenate(ea) if ea else np.zeros(0, np.int64)
        eb = np.concatenate(eb) if eb else np.zeros(0, np.int64)
        self.ea, self.eb = ea, eb
        pkey = rnd(P)
        self.sum_schur = OwnerSum(ecol[ea] * max(self.nf, 1) + ecol[eb], pkey[pb.ept[ea]], self.nf * self.nf)
        self.sum_coef = OwnerSum(ecol[pe], pkey[pb.ept[pe]], self.nf)
        self.perm_e = None if order is None else order.permutation(E)
        self.perm_v = None if order is None else order.permutation(K + P)
        self.ecol = ecol

    def chi(self, rho0):
        return _seqsum(np.where(self.active, rho0, 0.0), self.perm_e)

    def linearize(self, ed):
        """-> Hll [P, 6], bl [P, 3], Hpp [nf, 21], bp [nf, 6], max |diagonal|"""
        pt = self.sum_pt(ed[self.ae][:, :9])
        po = self.sum_pose(ed[self.pe][:, 9:36])
        self.Hll, self.bl, self.Hpp, self.bp = pt[:, :6], pt[:, 6:], po[:, :21], po[:, 21:]
        self.W = ed[:, 36:].reshape(-1, 6, 3)
        # computeLambdaInit, optimization_algorithm_levenberg.cpp:171-178: maxDiagonal = std::max(fabs(h), maxDiagonal) over the poses'
        # diagonals, then the points'.  std::max(a, b) is (a < b) ? b : a, so a NaN h replaces the running maximum and the next h
        # replaces the NaN: the maximum over the entries after the last NaN, NaN when the last entry is one
        diag = np.concatenate([np.abs(self.Hpp[:, DIAG6]).reshape(-1), np.abs(self.Hll[self.pact][:, DIAG3]).reshape(-1)])
        md = 0.0
        for a in diag.tolist():
            md = md if a < md else a
        return md

    def solve(self, lam):
        """one trial's linear step -> (ok, xp [nf, 6], xl [P, 3]); x = 0 after a bad pivot.  (g2o's x then is what the solve before
        left - block_solver.hpp:447-457 returns before writing it - and at a call's first solve what `new double[]` held,
        solver.cpp:54: uninitialised memory.  Zero is the kernels' deterministic choice, as for a never-evaluated edge's chi2;
        computeScale below still runs over every entry, so a non-finite b makes the scale NaN as :185-187 would with x = 0.)"""
        pb, nf, W = self.pb, self.nf, self.W
        with np.errstate(all="ignore"):
            H = self.Hll
            a00, a01, a02, a11, a12, a22 = H[:, 0] + lam, H[:, 1], H[:, 2], H[:, 3] + lam, H[:, 4], H[:, 5] + lam
            c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
            c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
            det = (a00 * c00 + a01 * c01) + a02 * c02
            idet = 1.0 / det
            i00, i01, i02, i11, i12, i22 = c00 * idet, c01 * idet, c02 * idet, c11 * idet, c12 * idet, c22 * idet
            Di = np.array([[i00, i01, i02], [i01, i11, i12], [i02, i12, i22]])      # [3, 3, P]
            b = self.bl
            db = np.stack([(i00 * b[:, 0] + i01 * b[:, 1]) + i02 * b[:, 2], (i01 * b[:, 0] + i11 * b[:, 1]) + i12 * b[:, 2],
                           (i02 * b[:, 0] + i12 * b[:, 1]) + i22 * b[:, 2]], 1)
            n = 6 * nf
            ok = True
            xp = np.zeros((nf, 6))
            if nf:
                ea, eb = self.ea, self.eb
                Wa, Wb, Dp = W[ea], W[eb], Di[:, :, pb.ept[ea]]
                Y = np.stack([(Wa[:, :, 0] * Dp[0, l] [:, None] + Wa[:, :, 1] * Dp[1, l][:, None]) + Wa[:, :, 2] * Dp[2, l][:, None] for l in range(3)], 2)
                term = (Y[:, :, None, 0] * Wb[:, None, :, 0] + Y[:, :, None, 1] * Wb[:, None, :, 1]) + Y[:, :, None, 2] * Wb[:, None, :, 2]
                acc = self.sum_schur(term).reshape(nf, nf, 6, 6)
                Wp, dbp = W[self.pe], db[pb.ept[self.pe]]
                coef = self.sum_coef((Wp[:, :, 0] * dbp[:, 0, None] + Wp[:, :, 1] * dbp[:, 1, None]) + Wp[:, :, 2] * dbp[:, 2, None])
                S = np.zeros((n, n))
                for i1 in range(nf):
                    for k, (j, l) in enumerate(UP6):
                        h = self.Hpp[i1, k] + lam if j == l else self.Hpp[i1, k]
                        S[6 * i1 + l, 6 * i1 + j] = h - acc[i1, i1, l, j]
                    for i2 in range(i1 + 1, nf):
                        S[6 * i2:6 * i2 + 6, 6 * i1:6 * i1 + 6] = (0.0 - acc[i1, i2]).T
                v = (self.bp - coef).reshape(n)
                self.S, self.bschur = S.copy(), v.copy()
                for m in range(n):
                    d = S[m, m]
                    if not (d > 0.0) or not (d <= DBL_MAX):
                        ok = False
                    S[m + 1:, m] = S[m + 1:, m] / d
                    L = S[m + 1:, m]
                    S[m + 1:, m + 1:] -= (L[:, None] * L[None, :]) * d
                for m in range(n):
                    v[m + 1:] -= S[m + 1:, m] * v[m]
                v = v / np.diag(S)
                for m in range(n - 1, -1, -1):
                    v[:m] -= S[m, :m] * v[m]
                xp = v.reshape(nf, 6) if ok else np.zeros((nf, 6))
            xl = np.zeros((pb.P, 3))
            if ok:
                pe = self.pe
                t = np.zeros((len(pe), 3))
                xe = xp[self.ecol[pe]]
                for j in range(6):
                    t += W[pe][:, j, :] * xe[:, j, None]
                cl = self.sum_back(t, init=self.bl, sign=-1)
                xl = np.stack([(i00 * cl[:, 0] + i01 * cl[:, 1]) + i02 * cl[:, 2], (i01 * cl[:, 0] + i11 * cl[:, 1]) + i12 * cl[:, 2],
                               (i02 * cl[:, 0] + i12 * cl[:, 1]) + i22 * cl[:, 2]], 1)
                xl[~self.pact] = 0.0
        return ok, xp, xl

    def scale(self, lam, xp, xl):
        """computeScale: sum x (lambda x + b), a vertex's coordinates first, then the vertices in order"""
        pb = self.pb
        terms = np.zeros(pb.K + pb.P)
        with np.errstate(all="ignore"):
            if self.nf:
                s = np.zeros(self.nf)
                for j in range(6):
                    s += xp[:, j] * (lam * xp[:, j] + self.bp[:, j])
                terms[self.kf_of_col] = s
            s = np.zeros(pb.P)
            for l in range(3):
                s += xl[:, l] * (lam * xl[:, l] + self.bl[:, l])
            terms[pb.K:] = np.where(self.pact, s, 0.0)
        return _seqsum(terms, self.perm_v)


def optimize(kfs, pts, obs, schedule=None, stop=None, order=None, perturb=None, exact_invz=False):
    """-> dict(Tcw [K, 4, 4] float32, pts [P, 3] float32, erase [E] uint8, kf_est [K, 7] (q, t), pt_est [P, 3], info, trace).
    stop: a callable polled where the reference reads pbStopFlag.  trace[r] = dict(iterations, trials, accepted, chis (the chi2 after
    every accepted trial, from the first linearisation's), min_abs_rho, and per iteration trials_it, rhos_it, tmps_it (the trial's
    chi2 as summed, before a failed solve makes it DBL_MAX) and oks_it (the solver's ok); ends: how the round's loop terminated);
    trace_class = per classification dict(min_margin, min_depth, flags, depth [E] = |z|)."""
    sc = schedule_local() if schedule is None else schedule
    pb = Problem(kfs, pts, obs, exact_invz)
    K, P, E = pb.K, pb.P, pb.E
    poses, points = pb.initial()
    flag = np.zeros(E, bool)
    last = np.zeros(E)
    info = dict(rounds=0, iterations=[0, 0], trials=[0, 0], free_poses=[0, 0], stopped_at=0, stop_poll=0, polls=0, erased=0)
    trace, trace_class = [], []

    def poll(where):
        if stop is None:
            return False
        info["polls"] += 1
        s = bool(stop())
        if s and not info["stopped_at"]:
            info["stopped_at"], info["stop_poll"] = where, info["polls"]
        return s

    def classify():
        _, _, z, _ = pb.camera_points(poses, points)
        with np.errstate(all="ignore"):
            out = (last > pb.thr) | ~(z > 0.0)
            trace_class.append(dict(min_margin=float(np.abs(last / pb.thr - 1.0).min()) if E else np.inf,
                                    min_depth=float(np.abs(z).min()) if E else np.inf, flags=out.copy(), depth=np.abs(z)))
        return out

    untouched = False
    do_classify = bool(sc["classify"])
    if sc["check_stop_first"] and poll(STOP_BEFORE):
        untouched, do_classify = True, False
    for rnd in range(sc["rounds"]):
        if untouched:
            break
        if rnd == 1:
            if poll(STOP_BETWEEN):
                break
            flag = classify()
        active = ~flag
        R = Round(pb, active, order)
        info["rounds"] = rnd + 1
        info["free_poses"][rnd] = R.nf
        tr = dict(iterations=0, trials=0, accepted=[], chis=[], min_abs_rho=np.inf, trials_it=[], rhos_it=[], tmps_it=[], oks_it=[], ends=[])
        trace.append(tr)
        if not active.any():
            continue
        robust = bool(sc["robust"][rnd])
        dM, dS = sc["delta_mono"], sc["delta_stereo"]
        where = STOP_ROUND1 if rnd == 0 else STOP_ROUND2
        lam, ni, nbad_it, ok_loop = 0.0, 2.0, 0, True
        for it in range(sc["iterations"][rnd]):
            if poll(where) or not ok_loop:
                break
            ev = pb.evaluate(poses, points, robust, dM, dS, True)
            last[active] = ev["chi2"][active]
            cur = R.chi(ev["rho0"])
            ini = cur
            md = R.linearize(ev["ed"])
            if it == 0:
                lam, ni, nbad_it = 1e-5 * md, 2.0, 0
                tr["chis"].append(cur)
            rho, q = 0.0, 0
            tr["rhos_it"].append([]); tr["tmps_it"].append([]); tr["oks_it"].append([])
            while True:
                ok, xp, xl = R.solve(lam)
                tposes, tpoints = poses.copy(), points.copy()
                if ok:
                    for c in range(R.nf):
                        k = R.kf_of_col[c]
                        tposes[k] = se3_oplus(poses[k], xp[c], perturb)
                    with np.errstate(all="ignore"):
                        tpoints = np.where(R.pact[:, None], points + xl, points)
                sc_ = R.scale(lam, xp, xl)
                ev = pb.evaluate(tposes, tpoints, robust, dM, dS, False)
                last[active] = ev["chi2"][active]
                tmp = R.chi(ev["rho0"])
                tr["tmps_it"][-1].append(tmp)
                tr["oks_it"][-1].append(ok)
                if not ok:
                    tmp = DBL_MAX
                with np.errstate(all="ignore"):
                    rho = (cur - tmp) / (sc_ + 1e-3)
                tr["min_abs_rho"] = min(tr["min_abs_rho"], abs(rho)) if rho == rho else 0.0
                tr["rhos_it"][-1].append(rho)
                if rho > 0.0 and abs(tmp) <= DBL_MAX:
                    u = 2.0 * rho - 1.0
                    alpha = min(1.0 - (u * u) * u, 2.0 / 3.0)
                    lam *= max(1.0 / 3.0, alpha)
                    ni = 2.0
                    cur = tmp
                    poses, points = tposes, tpoints
                    tr["accepted"].append(True)
                    tr["chis"].append(cur)
                else:
                    lam *= ni
                    ni *= 2.0
                    tr["accepted"].append(False)
                q += 1
                more = rho < 0.0 and q < MAX_TRIALS
                if more and poll(where):
                    more = False
                if not more:
                    break
            tr["iterations"] += 1
            tr["trials"] += q
            tr["trials_it"].append(q)
            info["iterations"][rnd], info["trials"][rnd] = tr["iterations"], tr["trials"]
            if q == MAX_TRIALS or rho == 0.0:
                ok_loop = False
                tr["ends"].append("qmax" if q == MAX_TRIALS else "rho0")
                continue
            nbad_it = nbad_it + 1 if (ini - cur) * 1e3 < ini else 0
            if nbad_it >= 3:
                ok_loop = False
                tr["ends"].append("nbad")
    erase = np.zeros(E, np.uint8)
    if do_classify:
        erase = classify().astype(np.uint8)
    info["erased"] = int(erase.sum())
    Tout = np.zeros((K, 4, 4), np.float32)
    for i in range(K):
        if pb.fixed[i] or untouched:
            Tout[i] = pb.kfs["Tcw"][i].reshape(4, 4)
        else:
            Tout[i, :3, :3] = quat_to_R(poses[i, 3:]).astype(np.float32)
            Tout[i, :3, 3] = poses[i, :3].astype(np.float32)
            Tout[i, 3, 3] = 1.0
    return dict(Tcw=Tout, pts=points.astype(np.float32), erase=erase, kf_est=np.concatenate([poses[:, 3:], poses[:, :3]], 1), pt_est=points.copy(),
                info=info, trace=trace, trace_class=trace_class, flag=flag.copy())
