"""Optimizer::OptimizeEssentialGraph (reference: src/Optimizer.cc:783-1049) and the g2o pieces it drives (types/sim3.h,
types_seven_dof_expmap.h, base_binary_edge.hpp's numeric linearizeOplus, block_solver.hpp without a Schur complement,
optimization_algorithm_levenberg with setUserLambdaInit(1e-16)), restated in numpy float64 ("k_eg_*").
Independent of the library: the GPU tests compare the kernels of csrc/orbx_essential.hip with this, the CPU tests check this against
properties and demand the kernels' text, run as one thread per workgroup, to give the same bytes.

Every sum has an owner and runs sequentially over the owner's terms in ascending input index; a caller may give a random generator
instead (`order`), which draws the order of every sum over edges (Hii, b, Hij, chi2) and over vertices (computeScale), so that the
effect of the summation order can be measured; `perturb` (a generator: the salt of a Perturb) moves every sin / cos / acos / log / exp by up to +-2 ulp, the same argument by the same amount.  The
elementary functions are the C library's (math.*), element by element: numpy's vector loops may round differently."""
import math

import numpy as np

DBL_MAX = np.finfo(np.float64).max
SIM3_DTYPE = np.dtype([("q", "<f8", (4,)), ("t", "<f8", (3,)), ("s", "<f8")])
VERTEX_DTYPE = np.dtype([("Scw", SIM3_DTYPE), ("Snc", SIM3_DTYPE), ("has_nc", "<i4"), ("fixed", "<i4")])
EDGE_DTYPE = np.dtype([("i", "<i4"), ("j", "<i4"), ("kind", "<i4")])
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("ref", "<i4")])
MAX_ITERATIONS, MAX_TRIALS, SLOTS, THREADS = 64, 10, 16, 1
END_ITERATIONS, END_QMAX, END_RHO0, END_SOLVER, END_NBAD = 0, 1, 2, 3, 4
EPS, DELTA = 0.00001, 1e-9


class Trace:
    """what the evaluations of one call came near: the smallest relative distance of |sigma|, theta and 1 - d from 1e-5 and of the
    3x3 solve's pivot from the runner-up; how often each branch of the exponential and of the logarithm was entered"""

    def __init__(self):
        self.margin = dict(sigma=np.inf, theta=np.inf, d=np.inf, pivot=np.inf)
        self.exp_branches, self.log_branches = np.zeros(4, np.int64), np.zeros(4, np.int64)
        self.iterations = []      # dict(chi2, rho [trials], margin) per iteration

    def near(self, what, value, thr):
        if len(value):
            self.margin[what] = min(self.margin[what], float(np.abs(np.asarray(value) / thr - 1.0).min()))

    def smallest(self):
        return min(self.margin.values())


class Perturb:
    """another C library: every elementary function's value moved by -2..+2 ulp, by an amount that depends on the argument's bits
    and on this object's salt alone - the same argument gives the same value, as on any one machine, so that differences which
    cancel exactly there (the two signs of a Jacobian step that oplusImpl zeroes) cancel exactly here"""

    def __init__(self, rng):
        self.salt = np.uint64(rng.integers(1, 2 ** 63)) | np.uint64(1)

    def ulps(self, x):
        with np.errstate(over="ignore"):
            h = (np.ascontiguousarray(x, np.float64).view(np.uint64) + self.salt) * np.uint64(0x9E3779B97F4A7C15)
            h ^= h >> np.uint64(29)
            h *= np.uint64(0xBF58476D1CE4E5B9)
        return ((h >> np.uint64(40)) % np.uint64(5)).astype(np.int64) - 2


def _fn(f, x, perturb):
    x = np.asarray(x, np.float64)
    r = np.array([f(float(v)) for v in x.reshape(-1)], np.float64).reshape(x.shape)
    if perturb is not None and r.size:
        r = r + perturb.ulps(x) * np.spacing(r)
    return r


def _masked(f, x, mask, perturb):
    """f over x where mask, 1.0 elsewhere (never used there)"""
    r = np.ones_like(x)
    if mask.any():
        r[mask] = _fn(f, x[mask], perturb)
    return r


# ---- Sim3 over arrays: q [n, 4] (x y z w), t [n, 3], s [n] -----------------------------------------------------------------------
def quat_from_R(R):
    """Eigen::Quaternion(Matrix3) (Shoemake), no normalisation; R [n, 3, 3]"""
    n = len(R)
    q = np.zeros((n, 4))
    with np.errstate(all="ignore"):
        tr = R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2]
        pos = tr > 0.0
        t = np.sqrt(tr + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q[pos, 3] = w[pos]
        q[pos, 0] = ((R[:, 2, 1] - R[:, 1, 2]) * t)[pos]
        q[pos, 1] = ((R[:, 0, 2] - R[:, 2, 0]) * t)[pos]
        q[pos, 2] = ((R[:, 1, 0] - R[:, 0, 1]) * t)[pos]
        for e in np.nonzero(~pos)[0]:
            M = R[e]
            i = 0
            if M[1, 1] > M[0, 0]:
                i = 1
            if M[2, 2] > M[i, i]:
                i = 2
            j, k = (i + 1) % 3, (i + 2) % 3
            t1 = np.sqrt(M[i, i] - M[j, j] - M[k, k] + 1.0)
            q[e, i] = 0.5 * t1
            t1 = 0.5 / t1
            q[e, 3] = (M[k, j] - M[j, k]) * t1
            q[e, j] = (M[j, i] + M[i, j]) * t1
            q[e, k] = (M[k, i] + M[i, k]) * t1
    return q


def quat_rotate(q, v):
    """Quaternion * Vector3 (_transformVector)"""
    uv0 = q[:, 1] * v[:, 2] - q[:, 2] * v[:, 1]
    uv1 = q[:, 2] * v[:, 0] - q[:, 0] * v[:, 2]
    uv2 = q[:, 0] * v[:, 1] - q[:, 1] * v[:, 0]
    uv0, uv1, uv2 = uv0 + uv0, uv1 + uv1, uv2 + uv2
    return np.stack([(v[:, 0] + q[:, 3] * uv0) + (q[:, 1] * uv2 - q[:, 2] * uv1),
                     (v[:, 1] + q[:, 3] * uv1) + (q[:, 2] * uv0 - q[:, 0] * uv2),
                     (v[:, 2] + q[:, 3] * uv2) + (q[:, 0] * uv1 - q[:, 1] * uv0)], 1)


def quat_to_R(q):
    """Quaternion::toRotationMatrix -> [n, 3, 3]"""
    tx, ty, tz = 2.0 * q[:, 0], 2.0 * q[:, 1], 2.0 * q[:, 2]
    twx, twy, twz = tx * q[:, 3], ty * q[:, 3], tz * q[:, 3]
    txx, txy, txz = tx * q[:, 0], ty * q[:, 0], tz * q[:, 0]
    tyy, tyz, tzz = ty * q[:, 1], tz * q[:, 1], tz * q[:, 2]
    R = np.zeros((len(q), 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = 1.0 - (tyy + tzz), txy - twz, txz + twy
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = txy + twz, 1.0 - (txx + tzz), tyz - twx
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = txz - twy, tyz + twx, 1.0 - (txx + tyy)
    return R


def mul(a, b):
    """Sim3::operator* (sim3.h:266-272); a, b = (q, t, s)"""
    aq, at, as_ = a
    bq, bt, bs = b
    ax, ay, az, aw = aq.T
    bx, by, bz, bw = bq.T
    q = np.stack([((aw * bx + ax * bw) + ay * bz) - az * by,
                  ((aw * by + ay * bw) + az * bx) - ax * bz,
                  ((aw * bz + az * bw) + ax * by) - ay * bx,
                  ((aw * bw - ax * bx) - ay * by) - az * bz], 1)
    rt = quat_rotate(aq, bt)
    return q, as_[:, None] * rt + at, as_ * bs


def inverse(a):
    """Sim3::inverse (sim3.h:233-236)"""
    q, t, s = a
    qi = np.stack([-q[:, 0], -q[:, 1], -q[:, 2], q[:, 3]], 1)
    k = -1. / s
    return qi, quat_rotate(qi, k[:, None] * t), 1. / s


def smap(a, p):
    """Sim3::map: s * (r * xyz) + t"""
    q, t, s = a
    return s[:, None] * quat_rotate(q, p) + t


def _skew2(o0, o1, o2):
    z = np.zeros_like(o0)
    Om = np.stack([np.stack([z, -o2, o1], 1), np.stack([o2, z, -o0], 1), np.stack([-o1, o0, z], 1)], 1)      # [n, 3, 3]
    Om2 = np.zeros_like(Om)
    for r in range(3):
        for c in range(3):
            Om2[:, r, c] = (Om[:, r, 0] * Om[:, 0, c] + Om[:, r, 1] * Om[:, 1, c]) + Om[:, r, 2] * Om[:, 2, c]
    return Om, Om2


def exp7(u, perturb=None, trace=None):
    """Sim3(const Vector7d &update) (sim3.h:70-142): u [n, 7] = omega | upsilon | sigma"""
    u = np.asarray(u, np.float64)
    o0, o1, o2, sigma = u[:, 0], u[:, 1], u[:, 2], u[:, 6]
    theta = np.sqrt((o0 * o0 + o1 * o1) + o2 * o2)
    Om, Om2 = _skew2(o0, o1, o2)
    s = _fn(math.exp, sigma, perturb)
    ss, st = np.abs(sigma) < EPS, theta < EPS
    if trace is not None:
        trace.near("sigma", np.abs(sigma), EPS)
        trace.near("theta", theta, EPS)
        for b, m in enumerate((ss & st, ss & ~st, ~ss & st, ~ss & ~st)):
            trace.exp_branches[b] += int(m.sum())
    si, co = _masked(math.sin, theta, ~st, perturb), _masked(math.cos, theta, ~st, perturb)
    with np.errstate(all="ignore"):
        theta2, sigma2 = theta * theta, sigma * sigma
        ra = np.where(st, 1.0, si / theta)
        rb = np.where(st, 1.0, (1.0 - co) / (theta * theta))
        Cc = np.where(ss, 1.0, (s - 1.0) / sigma)
        a, b, c = s * si, s * co, theta2 + sigma2
        A = np.where(ss, np.where(st, 1. / 2., (1.0 - co) / theta2),
                     np.where(st, ((sigma - 1.0) * s + 1.0) / sigma2, (a * sigma + (1.0 - b) * theta) / (theta * c)))
        B = np.where(ss, np.where(st, 1. / 6., (theta - si) / (theta2 * theta)),
                     np.where(st, ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma), ((Cc - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2))
    I = np.eye(3)[None]
    R = (I + ra[:, None, None] * Om) + rb[:, None, None] * Om2
    W = (A[:, None, None] * Om + B[:, None, None] * Om2) + Cc[:, None, None] * I
    t = np.stack([(W[:, r, 0] * u[:, 3] + W[:, r, 1] * u[:, 4]) + W[:, r, 2] * u[:, 5] for r in range(3)], 1)
    return quat_from_R(R), t, s


def lu3_solve(W, t, trace=None):
    """W.lu().solve(t), 3x3, partial pivoting: in column k the row of the largest |entry| among rows k.., the first on a tie"""
    W, b = W.copy(), t.copy()
    n = len(W)
    ar = np.arange(n)
    with np.errstate(all="ignore"):
        for k in range(3):
            a = np.abs(W[:, k:, k])
            p = k + np.argmax(a, 1)                  # the first of the largest
            if trace is not None and n and a.shape[1] > 1:
                srt = np.sort(a, 1)
                trace.near("pivot", srt[:, -2] / srt[:, -1], 1.0)      # the runner-up against the pivot
            rk, rp = W[ar, k].copy(), W[ar, p].copy()
            W[ar, k], W[ar, p] = rp, rk
            bk, bp = b[ar, k].copy(), b[ar, p].copy()
            b[ar, k], b[ar, p] = bp, bk
            piv = W[:, k, k].copy()
            for r in range(k + 1, 3):
                W[:, r, k] = W[:, r, k] / piv
                for c in range(k + 1, 3):
                    W[:, r, c] -= W[:, r, k] * W[:, k, c]
        b[:, 1] -= W[:, 1, 0] * b[:, 0]
        b[:, 2] -= W[:, 2, 0] * b[:, 0]
        b[:, 2] -= W[:, 2, 1] * b[:, 1]
        x2 = b[:, 2] / W[:, 2, 2]
        x1 = (b[:, 1] - W[:, 1, 2] * x2) / W[:, 1, 1]
        x0 = ((b[:, 0] - W[:, 0, 1] * x1) - W[:, 0, 2] * x2) / W[:, 0, 0]
    return np.stack([x0, x1, x2], 1)


def log7(S, perturb=None, trace=None, fixed_line_199=False):
    """Sim3::log (sim3.h:148-230) -> [n, 7] = omega | upsilon | sigma.  fixed_line_199: the branch |sigma| >= eps, d > 1 - eps with the
    '- 1' line 199 lacks - NOT the reference, only for the test that shows what the reference's formula does"""
    q, t, s = S
    sigma = _fn(math.log, s, perturb)
    R = quat_to_R(q)
    d = 0.5 * (((R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]) - 1.0)
    dR = np.stack([R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]], 1)
    ss, sd = np.abs(sigma) < EPS, d > 1.0 - EPS
    if trace is not None:
        trace.near("sigma", np.abs(sigma), EPS)
        trace.near("d", 1.0 - d, EPS)
        for b, m in enumerate((ss & sd, ss & ~sd, ~ss & sd, ~ss & ~sd)):
            trace.log_branches[b] += int(m.sum())
    theta = _masked(math.acos, np.where(sd, 0.5, d), ~sd, perturb)
    si, co = _masked(math.sin, theta, ~sd, perturb), _masked(math.cos, theta, ~sd, perturb)
    with np.errstate(all="ignore"):
        theta2, sigma2 = theta * theta, sigma * sigma
        k = np.where(sd, 0.5, theta / (2.0 * np.sqrt(1.0 - d * d)))
        Cc = np.where(ss, 1.0, (s - 1.0) / sigma)
        a, b, c = s * si, s * co, theta2 + sigma * sigma
        B199 = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma)
        if fixed_line_199:
            B199 = ((0.5 * sigma2 - sigma + 1.0) * s - 1.0) / (sigma2 * sigma)
        A = np.where(ss, np.where(sd, 1. / 2., (1.0 - co) / theta2),
                     np.where(sd, ((sigma - 1.0) * s + 1.0) / sigma2, (a * sigma + (1.0 - b) * theta) / (theta * c)))
        B = np.where(ss, np.where(sd, 1. / 6., (theta - si) / (theta2 * theta)),
                     np.where(sd, B199, ((Cc - ((b - 1.0) * sigma + a * theta) / c) * 1.) / theta2))
    o0, o1, o2 = k * dR[:, 0], k * dR[:, 1], k * dR[:, 2]
    Om, Om2 = _skew2(o0, o1, o2)
    W = (A[:, None, None] * Om + B[:, None, None] * Om2) + Cc[:, None, None] * np.eye(3)[None]
    ups = lu3_solve(W, t, trace)
    return np.concatenate([np.stack([o0, o1, o2], 1), ups, sigma[:, None]], 1)


def edge_error(Cm, Si, Sj, perturb=None, trace=None, **kw):
    """EdgeSim3::computeError: (C * v1 * v2^-1).log()"""
    return log7(mul(mul(Cm, Si), inverse(Sj)), perturb, trace, **kw)


def _rec(a):
    a = np.asarray(a)
    return a["q"].astype(np.float64).reshape(-1, 4), a["t"].astype(np.float64).reshape(-1, 3), a["s"].astype(np.float64).reshape(-1)


def _take(S, idx):
    return S[0][idx], S[1][idx], S[2][idx]


# ---- the symbolic half --------------------------------------------------------------------------------------------------------
class Symbolic:
    """natural order of the free vertices (not fixed, with an edge); elimination tree; the factor's block pattern with fill; per
    block the updates in ascending column; the levels"""

    def __init__(self, fixed, ei, ej, N):
        E = len(ei)
        has = np.zeros(N, bool)
        has[ei] = True
        has[ej] = True
        free = has & ~fixed
        self.vtxOfCol = np.nonzero(free)[0]
        self.nf = nf = len(self.vtxOfCol)
        self.colOf = np.full(N, -1, np.int64)
        self.colOf[self.vtxOfCol] = np.arange(nf)
        ci, cj = self.colOf[ei], self.colOf[ej]
        self.vEdges = [[] for _ in range(nf)]             # (edge, side) ascending edge
        pair_edges = {}
        for e in range(E):
            if ci[e] >= 0:
                self.vEdges[ci[e]].append((e, 0))
            if cj[e] >= 0:
                self.vEdges[cj[e]].append((e, 1))
            if ci[e] >= 0 and cj[e] >= 0:
                c, r = min(ci[e], cj[e]), max(ci[e], cj[e])
                pair_edges.setdefault((c, r), []).append((e, 0 if ci[e] == r else 1))      # the side of the ROW vertex
        self.pairs = sorted(pair_edges)                   # (column, row) lexicographic
        self.pair_edges = [pair_edges[p] for p in self.pairs]
        self.noff = len(self.pairs)
        st = [[] for _ in range(nf)]
        for c, r in self.pairs:
            st[c].append(r)
        fs = [sorted(set(x)) for x in st]
        self.parent, self.level = np.full(nf, -1, np.int64), np.zeros(nf, np.int64)
        for c in range(nf):
            fs[c] = sorted(set(fs[c]))
            if not fs[c]:
                continue
            p = fs[c][0]
            self.parent[c] = p
            fs[p] = fs[p] + fs[c][1:]
            self.level[p] = max(self.level[p], self.level[c] + 1)
        self.struct = fs
        self.colStart = np.concatenate([[0], np.cumsum([1 + len(x) for x in fs])]).astype(np.int64)
        self.nblk = int(self.colStart[-1])
        self.blkRow, self.blkCol, self.blkSrc = np.zeros(self.nblk, np.int64), np.zeros(self.nblk, np.int64), np.full(self.nblk, -1, np.int64)
        pidx = {p: i for i, p in enumerate(self.pairs)}
        self.blk = {}
        self.rows = [[] for _ in range(nf)]               # per column c: the blocks (c, k), k ascending
        for c in range(nf):
            b = int(self.colStart[c])
            self.blkRow[b], self.blkCol[b] = c, c
            self.blk[(c, c)] = b
            for k, r in enumerate(fs[c]):
                self.blkRow[b + 1 + k], self.blkCol[b + 1 + k] = r, c
                self.blkSrc[b + 1 + k] = pidx.get((c, r), -1)
                self.blk[(r, c)] = b + 1 + k
                self.rows[r].append(b + 1 + k)
        # per column c and source column k < c (ascending): the column's blocks that take the update, and their sources
        self.updates = []
        for c in range(nf):
            lst = []
            for bc in self.rows[c]:
                k = int(self.blkCol[bc])
                dst, srcA = [], []
                for b in range(int(self.colStart[c]), int(self.colStart[c + 1])):
                    r = int(self.blkRow[b])
                    ba = bc if r == c else self.blk.get((r, k))
                    if ba is not None:
                        dst.append(b)
                        srcA.append(ba)
                lst.append((np.array(dst), np.array(srcA), bc, int(self.colStart[k])))
            self.updates.append(lst)
        self.nlev = int(self.level.max()) + 1 if nf else 0
        self.levels = [np.nonzero(self.level == l)[0] for l in range(self.nlev)]


def factor_solve(sym, Hd, Hoff, b, lam):
    """(Hpp + lambda I) x = b by the block LDL^T of k_eg_assemble / k_eg_factor / k_eg_forward / k_eg_backward, statement for
    statement -> (x [nf, 7], ok, L [nblk, 7, 7])"""
    nf = sym.nf
    L = np.zeros((sym.nblk, 7, 7))
    diag = sym.colStart[:-1]
    L[diag] = Hd
    L[diag, np.arange(7)[:, None], np.arange(7)[:, None]] += lam
    src = sym.blkSrc >= 0
    L[src] = Hoff[sym.blkSrc[src]]
    ok = True
    with np.errstate(all="ignore"):
        for lev in sym.levels:
            for c in lev:
                b0, b1 = int(sym.colStart[c]), int(sym.colStart[c + 1])
                for dst, srcA, bc, dk in sym.updates[c]:
                    Lb, dd = L[bc], np.diagonal(L[dk])
                    for m in range(7):
                        L[dst] -= (L[srcA][:, :, m] * dd[m])[:, :, None] * Lb[None, None, :, m]
                A = L[b0]
                Dg = np.zeros((7, 7))
                for j in range(7):
                    v = A[j, j]
                    for m in range(j):
                        v -= (Dg[j, m] * Dg[m, m]) * Dg[j, m]
                    if not (v > 0.0) or not (v <= DBL_MAX):
                        ok, v = False, 1.0
                    Dg[j, j] = v
                    for i in range(j + 1, 7):
                        w = A[i, j]
                        for m in range(j):
                            w -= (Dg[i, m] * Dg[m, m]) * Dg[j, m]
                        Dg[i, j] = w / v
                for j in range(7):
                    A[j:, j] = Dg[j:, j]
                if b1 > b0 + 1:
                    rows = L[b0 + 1:b1]                       # [nb - 1, 7, 7]
                    xr = np.zeros_like(rows)
                    for bb in range(7):
                        v = rows[:, :, bb].copy()
                        for m in range(bb):
                            v -= (xr[:, :, m] * Dg[m, m]) * Dg[bb, m]
                        xr[:, :, bb] = v / Dg[bb, bb]
                    L[b0 + 1:b1] = xr
        x = b.copy()
        for lev in sym.levels:
            for c in lev:
                y = x[c].copy()
                for blk in sym.rows[c]:
                    Lb, yk = L[blk], x[sym.blkCol[blk]]
                    for m in range(7):
                        y -= Lb[:, m] * yk[m]
                Lc = L[sym.colStart[c]]
                for a in range(1, 7):
                    for m in range(a):
                        y[a] -= Lc[a, m] * y[m]
                x[c] = y
        for lev in sym.levels[::-1]:
            for c in lev:
                b0, b1 = int(sym.colStart[c]), int(sym.colStart[c + 1])
                Lc = L[b0]
                xc = x[c] / np.diagonal(Lc)
                for blk in range(b0 + 1, b1):
                    Lb, xr = L[blk], x[sym.blkRow[blk]]
                    for m in range(7):
                        xc -= Lb[m, :] * xr[m]
                for a in range(5, -1, -1):
                    for m in range(6, a, -1):
                        xc[a] -= Lc[m, a] * xc[m]
                x[c] = xc
    return x, ok, L


def _seqsum(a, perm=None):
    if len(a) == 0:
        return 0.0
    return float(np.cumsum(a if perm is None else a[perm])[-1])


class Problem:
    def __init__(self, vertices, edges, points, fix_scale):
        self.vtx, self.edges, self.pts = np.asarray(vertices, VERTEX_DTYPE), np.asarray(edges, EDGE_DTYPE), np.asarray(points, POINT_DTYPE)
        self.N, self.E, self.P = len(self.vtx), len(self.edges), len(self.pts)
        self.fix_scale = bool(fix_scale)
        self.ei, self.ej = self.edges["i"].astype(np.int64), self.edges["j"].astype(np.int64)
        self.fixed = self.vtx["fixed"] != 0
        self.Scw, self.Snc = _rec(self.vtx["Scw"]), _rec(self.vtx["Snc"])
        self.sym = Symbolic(self.fixed, self.ei, self.ej, self.N)
        nc = self.edges["kind"] != 0
        hi, hj = nc & (self.vtx["has_nc"][self.ei] != 0), nc & (self.vtx["has_nc"][self.ej] != 0)
        Siw = tuple(np.where(hi.reshape((-1,) + (1,) * (a.ndim - 1)), b[self.ei], a[self.ei]) for a, b in zip(self.Scw, self.Snc))
        Sjw = tuple(np.where(hj.reshape((-1,) + (1,) * (a.ndim - 1)), b[self.ej], a[self.ej]) for a, b in zip(self.Scw, self.Snc))
        self.meas = mul(Sjw, inverse(Siw)) if self.E else (np.zeros((0, 4)), np.zeros((0, 3)), np.zeros(0))

    def errors(self, est, perturb=None, trace=None, **kw):
        return edge_error(self.meas, _take(est, self.ei), _take(est, self.ej), perturb, trace, **kw)

    def step(self, col, sign):
        u = np.zeros((1, 7))
        u[0, col] = -DELTA if sign else DELTA
        if self.fix_scale:
            u[0, 6] = 0.0
        return u

    def jacobians(self, est, perturb=None, trace=None, delta=DELTA, **kw):
        """linearizeOplus -> J [E, 2, 7 (residual), 7 (column)]; the side of a fixed vertex stays zero (it is never read)"""
        J = np.zeros((self.E, 2, 7, 7))
        Si, Sj = _take(est, self.ei), _take(est, self.ej)
        scalar = 1.0 / (2 * delta)
        for side in range(2):
            use = ~self.fixed[self.ej if side else self.ei]
            for col in range(7):
                e2 = []
                for sign in range(2):
                    u = np.zeros((1, 7))
                    u[0, col] = -delta if sign else delta
                    if self.fix_scale:
                        u[0, 6] = 0.0
                    X = exp7(u, perturb, trace)
                    X = tuple(np.repeat(a, self.E, 0) for a in X)
                    Sp = mul(X, Sj if side else Si)
                    e2.append(edge_error(self.meas, Si if side else Sp, Sp if side else Sj, perturb, trace, **kw))
                J[use, side, :, col] = (scalar * (e2[0] - e2[1]))[use]
        return J

    def quadratic(self, J, err, order=None):
        """-> Hd [nf, 7, 7], b [nf, 7], Hoff [noff, 7, 7]: every owner's edges in ascending input index (or in a drawn order)"""
        sym = self.sym
        Hd, b, Hoff = np.zeros((sym.nf, 7, 7)), np.zeros((sym.nf, 7)), np.zeros((sym.noff, 7, 7))

        def inner(A, B):      # sum_k A[k, r] * B[k, c], k ascending
            t = A[0][:, None] * B[0][None, :]
            for k in range(1, 7):
                t = t + A[k][:, None] * B[k][None, :]
            return t
        for c in range(sym.nf):
            lst = sym.vEdges[c]
            if order is not None:
                lst = [lst[i] for i in order.permutation(len(lst))]
            for e, side in lst:
                A = J[e, side]
                Hd[c] += inner(A, A)
                t = A[0] * (-err[e, 0])
                for k in range(1, 7):
                    t = t + A[k] * (-err[e, k])
                b[c] += t
        for o in range(sym.noff):
            lst = sym.pair_edges[o]
            if order is not None:
                lst = [lst[i] for i in order.permutation(len(lst))]
            for e, sr in lst:
                Hoff[o] += inner(J[e, sr], J[e, sr ^ 1])
        return Hd, b, Hoff


def launches(sym, N, E, P, iterations, trials):
    """kernel launches of a call that ran `iterations` iterations and `trials` trials in all (eg_drive)"""
    n = 2 if max(N, E, P) > 0 else 0
    return n + iterations * (3 + (1 if sym.noff else 0)) + trials * (4 + 3 * sym.nlev)


def optimize(vertices, edges, points, fix_scale, iterations=20, order=None, perturb=None, **kw):
    """-> dict(Tcw [N, 4, 4] float32, pts [P, 3] float32, est [N, 8], info, trace)"""
    pr = Problem(vertices, edges, points, fix_scale)
    sym, N, E, P = pr.sym, pr.N, pr.E, pr.P
    assert 0 <= iterations <= MAX_ITERATIONS
    tr = Trace()
    if perturb is not None and not isinstance(perturb, Perturb):
        perturb = Perturb(perturb)
    est = tuple(a.copy() for a in pr.Scw)
    info = dict(iterations=0, trials=0, end=END_ITERATIONS, free_vertices=sym.nf, blocks=sym.nblk, levels=sym.nlev, launches=0, pad=0,
                chi2_first=0.0, chi2_last=0.0, trials_it=[0] * MAX_ITERATIONS)
    lam, ni, cur, nbad, ok, last_ok = 0.0, 2.0, 0.0, 0, True, True
    for it in range(iterations):
        if not ok or E == 0 or sym.nf == 0:
            break
        err = pr.errors(est, perturb, tr, **kw)
        chis = np.zeros(E)
        for k in range(7):
            chis = chis + err[:, k] * err[:, k]
        lin_chi = _seqsum(chis, None if order is None else order.permutation(E))
        J = pr.jacobians(est, perturb, tr, **kw)
        Hd, b, Hoff = pr.quadratic(J, err, order)
        if it == 0:
            lam, ni, nbad = 1e-16, 2.0, 0
        q, rho, ini = 0, 0.0, 0.0
        rhos, tmps, oks = [], [], []
        while True:
            x, last_ok, _ = factor_solve(sym, Hd, Hoff, b, lam)
            trial = tuple(a.copy() for a in est)
            sc = np.zeros(N)
            if last_ok:
                xs = x.copy()
                if pr.fix_scale:
                    xs[:, 6] = 0.0
                for j in range(7):
                    sc[sym.vtxOfCol] += xs[:, j] * (lam * xs[:, j] + b[:, j])
                new = mul(exp7(xs, perturb, tr), _take(est, sym.vtxOfCol))
                for a, n_ in zip(trial, new):
                    a[sym.vtxOfCol] = n_
            terr = pr.errors(trial, perturb, tr, **kw)
            tch = np.zeros(E)
            for k in range(7):
                tch = tch + terr[:, k] * terr[:, k]
            tmp = _seqsum(tch, None if order is None else order.permutation(E))
            scale = _seqsum(sc, None if order is None else order.permutation(N)) + 1e-3
            if q == 0:
                cur = ini = lin_chi
                if it == 0:
                    info["chi2_first"] = cur
            tmps.append(tmp); oks.append(last_ok)
            if not last_ok:
                tmp = DBL_MAX
            with np.errstate(all="ignore"):
                rho = float((np.float64(cur) - np.float64(tmp)) / np.float64(scale))
            rhos.append(rho)
            if rho > 0.0 and abs(tmp) <= DBL_MAX:
                u = 2.0 * rho - 1.0
                alpha = 1.0 - (u * u) * u
                alpha = min(alpha, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                cur = tmp
                est = trial
            else:
                lam *= ni
                ni *= 2.0
            q += 1
            if not (rho < 0.0 and q < MAX_TRIALS):
                break
        info["trials_it"][info["iterations"]] = q
        info["iterations"] += 1
        info["trials"] += q
        tr.iterations.append(dict(chi2=ini, chi2_after=cur, rho=rhos, tmp=tmps, ok=oks))
        if q == MAX_TRIALS or rho == 0.0:
            ok = False
            info["end"] = END_SOLVER if not last_ok else END_QMAX if q == MAX_TRIALS else END_RHO0
            continue
        nbad = nbad + 1 if (ini - cur) * 1e3 < ini else 0
        if nbad >= 3:
            ok = False
            info["end"] = END_NBAD
    info["chi2_last"] = cur
    info["launches"] = launches(sym, N, E, P, info["iterations"], info["trials"])
    q, t, s = est
    R = quat_to_R(q)
    Tcw = np.zeros((N, 4, 4), np.float32)
    Tcw[:, :3, :3] = R.astype(np.float32)
    Tcw[:, :3, 3] = (t * (1. / s)[:, None]).astype(np.float32)
    Tcw[:, 3, 3] = 1.0
    ref = pr.pts["ref"].astype(np.int64)
    X = np.stack([pr.pts["x"], pr.pts["y"], pr.pts["z"]], 1).astype(np.float64).reshape(P, 3)
    Xw = smap(inverse(_take(est, ref)), smap(_take(pr.Scw, ref), X)) if P else np.zeros((0, 3))
    return dict(Tcw=Tcw, pts=Xw.astype(np.float32), est=np.concatenate([q, t, s[:, None]], 1), info=info, trace=tr)
