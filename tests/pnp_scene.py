"""Seeded relocalisation scenes for the PnPsolver tests: map points seen by one camera.  Depth 3-9, intrinsics 500 / 500 / 320 / 240,
sigma2 = 1.2^(2 l) with l in 0..7, pixel noise in units of the level's scale, gross outliers at uniform pixels.  RANSAC parameters
are Relocalization's (0.99, 10, 300, 4, 0.5f, 5.991f) unless a scene says otherwise.  The shapes are the smallest that reach each
path of csrc/orbx_pnp.hip (CASES)."""
import numpy as np

import pnp_ref as R

K = (500.0, 500.0, 320.0, 240.0)
TH2 = 5.991
LEVEL_SIGMA2 = (np.float32(1.2) ** (2 * np.arange(8))).astype(np.float32)
_cache = {}


def rodrigues(axis, ang):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(ang) * Kx + (1 - np.cos(ang)) * Kx @ Kx


def pose(rng):
    T = np.eye(4)
    T[:3, :3] = rodrigues(rng.normal(size=3), rng.uniform(0.1, 0.6))
    T[:3, 3] = rng.uniform(-2, 2, 3)
    return T


def project(T, Xw):
    Xc = Xw @ T[:3, :3].T + T[:3, 3]
    return np.stack([K[0] * Xc[:, 0] / Xc[:, 2] + K[2], K[1] * Xc[:, 1] / Xc[:, 2] + K[3]], axis=1)


def make(seed, n, noise=0.5, outliers=0.3, min_inliers=10, epsilon=0.5, iterations=None, planar=False, T=None):
    """n correspondences: Xc at depth 3-9 inside the image, the keypoint = its projection + noise * 1.2^level pixels per axis, a
    share of gross outliers (a keypoint anywhere in the image)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K
    T = pose(rng) if T is None else T
    z = rng.uniform(3, 9, n)
    u, v = rng.uniform(40, 600, n), rng.uniform(40, 440, n)
    Xc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)
    Xw = (Xc - T[:3, 3]) @ T[:3, :3]
    if planar:                                    # coplanar in the WORLD: z_w = 1 - 0.2 x_w + 0.1 y_w, seen obliquely
        Xw[:, 2] = 1.0 - 0.2 * Xw[:, 0] + 0.1 * Xw[:, 1]
    lv = rng.integers(0, 8, n)
    corrs = np.zeros(n, R.CORR_DTYPE)
    corrs["w"] = Xw
    uv = project(T, corrs["w"].astype(np.float64)) + rng.normal(0, 1, (n, 2)) * (noise * 1.2 ** lv)[:, None]
    out = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k:
        out[rng.choice(n, k, replace=False)] = True
        uv[out] = np.stack([rng.uniform(0, 640, k), rng.uniform(0, 480, k)], axis=1)
    corrs["u"], corrs["v"], corrs["sigma2"] = uv[:, 0], uv[:, 1], LEVEL_SIGMA2[lv]
    mi, mx = R.pnp_parameters(n, 0.99, min_inliers, 300, 4, epsilon)
    its = (mx if n >= mi else 0) if iterations is None else iterations
    sets = R.draw_sets(n, its, lambda lo, hi: int(rng.integers(lo, hi + 1))) if n >= 4 else np.zeros((0, 4), np.int32)
    return dict(corrs=corrs, K=K, th2=TH2, min_inliers=mi, max_iterations=mx, sets=sets, iterations_done=0, prior_best_inliers=0,
                prior_best_flags=None, Tcw_true=T, outlier=out, level=lv, noise=noise, rng=rng)


def refine_fails_then_hits(seed):
    """60 correspondences, min_inliers 20 (epsilon 0.3): 20 exact ones of pose A, 40 exact ones of pose B.  Set 1 names four of A: a
    record of 20 whose refinement counts 20, not more; set 3 names four of B: the next record, whose refinement hits."""
    rng = np.random.default_rng(seed)
    a = make(seed, 20, noise=0.0, outliers=0.0, min_inliers=20, epsilon=0.3)
    b = make(seed + 100, 40, noise=0.0, outliers=0.0, min_inliers=20, epsilon=0.3)
    sc = dict(a, corrs=np.concatenate([a["corrs"], b["corrs"]]), outlier=np.zeros(60, bool), level=np.concatenate([a["level"], b["level"]]))
    sc["min_inliers"], sc["max_iterations"] = R.pnp_parameters(60, 0.99, 20, 300, 4, 0.3)
    sc["Tcw_true"] = b["Tcw_true"]
    mixed = lambda: np.array([rng.integers(0, 20), rng.integers(0, 20) , rng.integers(20, 60), rng.integers(20, 60)])   # noqa: E731
    sets = [mixed(), rng.choice(20, 4, replace=False), mixed(), 20 + rng.choice(40, 4, replace=False), mixed(), mixed()]
    for s in (sets[0], sets[2], sets[4], sets[5]):
        while s[0] == s[1] or s[2] == s[3]:
            s[1], s[3] = rng.integers(0, 20), rng.integers(20, 60)
    sc["sets"] = np.array(sets, np.int32)
    return sc


def behind(seed):
    """correspondences 5 and 6 lie behind the camera (z <= 0): projected without a guard, as the reference does"""
    sc = make(seed, 40)
    T = sc["Tcw_true"]
    for i, xc in ((5, [0.3, -0.2, -2.0]), (6, [-0.5, 0.4, -4.0])):
        sc["corrs"]["w"][i] = (np.array(xc) - T[:3, 3]) @ T[:3, :3]
        sc["outlier"][i] = True
    return sc


def duplicate(seed):
    """correspondence 1 is a copy of correspondence 0 and set 0 names both: three distinct points, a degenerate model"""
    sc = make(seed, 40, iterations=6)
    sc["corrs"][1] = sc["corrs"][0]
    sc["sets"][0] = (0, 1, 2, 3)
    return sc


def second_call(first, seed):
    """the scene of the call that follows a hit: the state the caller carries, and fresh sets"""
    sc, r = case(first), reference(first)
    rng = np.random.default_rng(seed)
    done = r["iterations_run"]
    its = max(sc["max_iterations"] - done, sc["max_iterations"])          # find(): nIterations = mRansacMaxIts
    return dict(sc, iterations_done=done, prior_best_inliers=int(r["best_inliers"]), prior_best_flags=r["best_flags"].copy(),
                sets=R.draw_sets(len(sc["corrs"]), its, lambda lo, hi: int(rng.integers(lo, hi + 1))))


# name -> constructor.  Seeds were picked from the restatement itself (tests/test_pnp_cpu.py asserts what each scene is for, and
# assert_conditions on every one).
CASES = {
    "n_4": lambda: make(0, 4, noise=0.0, outliers=0.0, min_inliers=4, iterations=5),
    "n_9": lambda: make(0, 9),
    "wave_63": lambda: make(3, 63, iterations=12),
    "wave_64": lambda: make(1, 64, iterations=12),
    "wave_65": lambda: make(2, 65, iterations=12),
    "n_257": lambda: make(7, 257, outliers=0.0, iterations=6),
    "n_1100": lambda: make(3, 1100, outliers=0.1, iterations=8),
    "hit_60": lambda: make(2, 60),
    "exact_40": lambda: make(0, 40, noise=0.0, outliers=0.0, iterations=12),
    "exhausted_60": lambda: make(7, 60, noise=0.0, outliers=0.5),    # 30 exact inliers = min_inliers: a refinement counts 30, never more
    "refine_fails_then_hits": lambda: refine_fails_then_hits(0),
    "two_calls": lambda: second_call("hit_60", 11),
    "planar": lambda: make(6, 50, planar=True, iterations=12),
    "behind": lambda: behind(0),
    "duplicate": lambda: duplicate(1),
}
BATCH_3 = ("hit_60", "n_9", "wave_65")        # n_9 runs no iteration; the empty problem is added between them


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name]()
    return _cache[name]


def reference(name):
    """the restatement's trace for a case, computed once and shared"""
    key = ("ref", name)
    if key not in _cache:
        sc = case(name)
        _cache[key] = R.ransac(sc["corrs"], sc["K"], sc["th2"], sc["min_inliers"], sc["max_iterations"], sc["sets"], sc["iterations_done"],
                               sc["prior_best_inliers"], sc["prior_best_flags"])
    return _cache[key]


def problem(sc):
    p = np.zeros(1, R.PROBLEM_DTYPE)
    p["K"], p["th2"], p["min_inliers"], p["max_iterations"] = sc["K"], sc["th2"], sc["min_inliers"], sc["max_iterations"]
    p["iterations_done"], p["prior_best_inliers"] = sc["iterations_done"], sc["prior_best_inliers"]
    return p


def prior_flags(sc):
    n = len(sc["corrs"])
    return np.zeros(n, np.uint8) if sc["prior_best_flags"] is None else np.ascontiguousarray(sc["prior_best_flags"], np.uint8)


def batch(names):
    """the scenes as one batched call, an EMPTY problem (no correspondences, no sets) after the first"""
    scs = [case(k) for k in names]
    scs.insert(1, dict(scs[0], corrs=scs[0]["corrs"][:0], sets=scs[0]["sets"][:0], prior_best_flags=None, prior_best_inliers=0))
    return pack_scenes(scs)


def pack_scenes(scs):
    off = np.cumsum([0] + [len(s["corrs"]) for s in scs]).astype(np.int32)
    soff = np.cumsum([0] + [len(s["sets"]) for s in scs]).astype(np.int32)
    return dict(scenes=scs, offsets=off, set_offsets=soff, problems=np.concatenate([problem(s) for s in scs]),
                corrs=np.concatenate([s["corrs"] for s in scs]), sets=np.concatenate([s["sets"] for s in scs]).astype(np.int32).reshape(-1, 4),
                prior=np.concatenate([prior_flags(s) for s in scs]))


def single(name):
    return pack_scenes([case(name)])


def pack(b):
    """the input file of tests/cpp/pnp_lockstep.cc"""
    return (np.int32(len(b["problems"])).tobytes() + b["offsets"].tobytes() + b["set_offsets"].tobytes() + b["problems"].tobytes() +
            b["corrs"].tobytes() + np.ascontiguousarray(b["sets"], np.int32).tobytes() + b["prior"].tobytes())


def unpack(b, buf):
    """the output file of the lockstep program -> per problem dict"""
    B, off, soff = len(b["problems"]), b["offsets"], b["set_offsets"]
    np_, nh = int(off[B]), int(soff[B])
    ns = nh + B
    o = [0]

    def take(dtype, count, shape=None):
        a = np.frombuffer(buf, dtype, count, o[0])
        o[0] += a.nbytes
        return a if shape is None else a.reshape(shape)
    infos = take(R.INFO_DTYPE, B)
    counts, choices, rcounts = take(np.int32, nh), take(np.int32, nh), take(np.int32, ns)
    inl, best = take(np.uint8, np_), take(np.uint8, np_)
    models, tcws = take(np.float64, nh * 12, (nh, 12)), take(np.float32, nh * 16, (nh, 4, 4))
    rmodels, rtcws = take(np.float64, ns * 12, (ns, 12)), take(np.float32, ns * 16, (ns, 4, 4))
    nfl = sum(int(soff[k + 1] - soff[k]) * int(off[k + 1] - off[k]) for k in range(B))
    nrf = sum(int(soff[k + 1] - soff[k] + 1) * int(off[k + 1] - off[k]) for k in range(B))
    flags, rflags = take(np.uint8, nfl), take(np.uint8, nrf)
    assert o[0] == len(buf)
    res, fb, rb = [], 0, 0
    for k in range(B):
        n, its = int(off[k + 1] - off[k]), int(soff[k + 1] - soff[k])
        h, r = slice(soff[k], soff[k + 1]), slice(soff[k] + k, soff[k + 1] + k + 1)
        res.append(dict(info=infos[k], counts=counts[h], choices=choices[h], rcounts=rcounts[r], inliers=inl[off[k]:off[k + 1]],
                        best_flags=best[off[k]:off[k + 1]], models=models[h], tcws=tcws[h], rmodels=rmodels[r], rtcws=rtcws[r],
                        flags=flags[fb:fb + its * n].reshape(its, n), rflags=rflags[rb:rb + (its + 1) * n].reshape(its + 1, n)))
        fb += its * n
        rb += (its + 1) * n
    return res


def same(a, b):
    """byte equality of float arrays of one type, a NaN equal to any NaN (its sign and payload are the platform's)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    ui = np.uint64 if a.dtype == np.float64 else np.uint32
    return bool(((a.view(ui) == b.view(ui)) | (np.isnan(a) & np.isnan(b))).all())


def assert_equals_restatement(o, r, full=True):
    """one problem's outputs against the restatement's trace.  full: the lockstep program's refined models, poses and flags too"""
    info = o["info"]
    for k in ("n", "iterations", "hit_iteration", "iterations_run", "best_iteration", "best_inliers", "refined_inliers", "no_more", "pose"):
        assert int(info[k]) == int(r[k]), (k, int(info[k]), int(r[k]))
    assert same(np.reshape(info["Tcw"], (4, 4)), r["Tcw"]) and same(np.reshape(info["best_Tcw"], (4, 4)), r["best_Tcw"])
    assert (o["inliers"] == r["inliers"]).all() and (o["best_flags"] == r["best_flags"]).all()
    if r["iterations"] and r["n"] >= 4 and r["rcounts"].size == o["rcounts"].size:
        live = not (r["no_more"] and r["iterations_run"] == 0)
        if live:
            assert (o["counts"] == r["counts"]).all() and (o["choices"] == r["choices"]).all() and (o["flags"] == r["flags"]).all()
            assert same(o["models"], r["models"]) and same(o["tcws"], r["tcws"])
            assert (o["rcounts"] == r["rcounts"]).all()
            if full:
                assert same(o["rmodels"], r["rmodels"]) and same(o["rtcws"], r["rtcws"]) and (o["rflags"] == r["rflags"]).all()


# ---- the conditions of the byte comparison (tests/test_pnp_cpu.py asserts them on the restatement alone)
def ulp32(x):
    x = np.abs(np.asarray(x, np.float32))
    return np.spacing(x).astype(np.float64)


def borderline(err, thr):
    """[.., n] bool: error2 lies within 4 float ulps of its threshold"""
    with np.errstate(invalid="ignore"):
        return np.abs(err.astype(np.float64) - thr.astype(np.float64)) <= 4 * ulp32(thr)


def assert_conditions(name):
    """at most 0.5 % of evaluations borderline; no count and no refined count that decides a branch lies within its iteration's
    borderline count of the value it is compared with (min_inliers, the best count so far)"""
    sc, r = case(name), reference(name)
    if not r["iterations"] or r["n"] < sc["min_inliers"]:
        return
    bl = borderline(r["err"], r["thr"][None])
    done = r["rcounts"] >= 0
    rbl = borderline(r["rerr"][done], r["thr"][None])
    total = bl.size + rbl.size
    assert bl.sum() + rbl.sum() <= 0.005 * total, "%s: %d of %d evaluations are borderline - choose another seed" % (name, bl.sum() + rbl.sum(), total)
    nb, mi = bl.sum(axis=1), sc["min_inliers"]
    best = sc["prior_best_inliers"]
    for it in range(r["iterations_run"]):
        c = int(r["counts"][it])
        assert nb[it] == 0 or not (c - nb[it] <= mi - 1 < c or c <= mi - 1 < c + nb[it]), "%s: iteration %d is within its borderline count of min_inliers" % (name, it)
        assert nb[it] == 0 or not (c - nb[it] <= best < c or c <= best < c + nb[it]), "%s: iteration %d is within its borderline count of the best" % (name, it)
        if c >= mi and c > best:
            best = c
    for s, nbs in zip(np.nonzero(done)[0], rbl.sum(axis=1)):
        c = int(r["rcounts"][s])
        assert nbs == 0 or not (c - nbs <= mi < c or c <= mi < c + nbs), "%s: slot %d is within its borderline count of min_inliers" % (name, s)
