"""Seeded two-view scenes for the Initializer tests: keys on a 640x480 image, K as the project's mono workloads use.  The shapes are
the smallest at which each part of csrc/orbx_initializer.hip can go wrong (see CASES)."""
import numpy as np

import init_ref as R

W, H = 640, 480
K4 = (517.3, 516.5, 318.6, 255.3)
_cache = {}


def rot(axis, deg):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def make(seed, N, kind="general", t=(0.3, 0.02, 0.01), deg=5.0, noise=0.5, outliers=0, iterations=64, extra1=0, extra2=0,
         sets="rng", plane=(4.0, 0.5, 0.3)):
    """N matched keypoints (+ extra1 / extra2 unmatched ones, all shuffled) of 3-D points seen from [I|0] and [R21|t21]"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K4
    R21, t21 = rot([0.1, 1.0, 0.05], deg), np.asarray(t, np.float64)
    p1, p2 = np.zeros((0, 2)), np.zeros((0, 2))
    while len(p1) < N:
        m = 4 * N
        uv = np.stack([rng.uniform(20, W - 20, m), rng.uniform(20, H - 20, m)], axis=1)
        ray = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(m)], axis=1)
        d = rng.uniform(2, 8, m) if kind != "planar" else plane[0] / (1 - plane[1] * ray[:, 0] - plane[2] * ray[:, 1])
        X = ray * d[:, None]
        X2 = X @ R21.T + t21
        uv2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], axis=1)
        ok = (X2[:, 2] > 0.5) & (uv2[:, 0] > 20) & (uv2[:, 0] < W - 20) & (uv2[:, 1] > 20) & (uv2[:, 1] < H - 20)
        p1, p2 = np.concatenate([p1, uv[ok]]), np.concatenate([p2, uv2[ok]])
    p1, p2 = p1[:N] + rng.normal(0, noise, (N, 2)), p2[:N] + rng.normal(0, noise, (N, 2))
    out = np.zeros(N, bool)
    if outliers:
        out[rng.choice(N, outliers, replace=False)] = True
        p2[out] = np.stack([rng.uniform(20, W - 20, outliers), rng.uniform(20, H - 20, outliers)], axis=1)
    n1, n2 = N + extra1, N + extra2
    k1 = np.concatenate([p1, np.stack([rng.uniform(0, W, extra1), rng.uniform(0, H, extra1)], axis=1)])
    k2 = np.concatenate([p2, np.stack([rng.uniform(0, W, extra2), rng.uniform(0, H, extra2)], axis=1)])
    perm1, perm2 = rng.permutation(n1), rng.permutation(n2)      # key i of the scene sits at perm[i]
    keys1, keys2 = np.zeros((n1, 2), np.float32), np.zeros((n2, 2), np.float32)
    keys1[perm1], keys2[perm2] = k1, k2
    order = np.argsort(perm1[:N])                                 # mvMatches12 is in ascending keypoint-1 index
    matches = np.stack([perm1[:N], perm2[:N]], axis=1)[order].astype(np.int32)
    if sets == "perm":                                            # every set a permutation of all (8) matches
        s = np.stack([rng.permutation(N)[:8] for _ in range(iterations)]).astype(np.int32)
    else:
        s = R.draw_sets(N, iterations, lambda lo, hi: int(rng.integers(lo, hi + 1)))
    return dict(keys1=keys1, keys2=keys2, matches=matches, sets=s, K4=K4, R_true=R21, t_true=t21, outlier=out[order], iterations=iterations,
                sigma=1.0, min_parallax=1.0, min_triangulated=50)


def redraw_sets(sc, seed):
    """the scene with its sets drawn again, from MT19937"""
    sc = dict(sc)
    rng = np.random.Generator(np.random.MT19937(seed))
    sc["sets"] = R.draw_sets(len(sc["matches"]), sc["iterations"], lambda lo, hi: int(rng.integers(lo, hi + 1)))
    return sc


def degenerate(seed):
    """all matches the same point pair (the keys themselves are distinct, so Normalize stays finite)"""
    sc = make(seed, 30, iterations=16)
    sc["matches"] = np.tile(sc["matches"][3], (20, 1)).astype(np.int32)
    sc["sets"] = R.draw_sets(20, 16, lambda lo, hi: lo)
    sc["outlier"] = np.zeros(20, bool)
    return sc


# name -> (constructor, what Initialize must answer: (result, model) with None = not stated).  The seeds are the first (from 200
# up; planar_120 from 1000 up) at which the restatement meets the four conditions tests/test_initializer_gpu.py asserts - about
# one seed in six does for a homography scene, whose wrong motions put many points at the 0.99998 test of CheckRT - and, for the
# first two, recovers the motion within the bounds of tests/test_initializer_cpu.py.  wg_257 / wg_257_mt: the same scene with sets
# from two generators (PCG64, MT19937).
# Past the LDS stages of csrc/orbx_initializer.hip (INI_CHUNK = 512 matches per pass of k_init_ransac, 2 x INI_CHUNK keys per pass
# of k_init_normalize) and past the 1 MiB floor of the staging pair - general scenes only: of planar scenes of 260, 300 and 513
# matches none of 400 seeds each met margin_rt.  Each seed is the first from 200 up at which the four conditions hold, whatever
# Initialize answers (seeds tried: 4, 3, 15, 1, 1, 6):
#   chunk_512        one full pass, cnt == INI_CHUNK                                               answers true
#   chunk_513        a second pass of one match; k_init_reconstruct strides 256 three times        answers true
#   chunk_1025       three passes (512 + 512 + 1); 1025 keys: two Normalize passes in both frames  answers true
#   keys_1024_1025   frame 1 exactly one Normalize pass, frame 2 one key more; 100 matches         answers false (23 points)
#   keys_2049_3000   three Normalize passes with different counts in the two frames                answers false (73 of 86 inliers)
#   regrow_513       2 x 1100 x 513 flag bytes > 1 MiB: the staging pair regrows; 2200 hypotheses  answers false (382 of 438 inliers)
CASES = {
    "general_150": (lambda: make(251, 150, outliers=30, iterations=200), (1, 1)),
    "planar_120": (lambda: make(1614, 120, kind="planar", outliers=20, iterations=200, plane=(2.5, 0.0, 1.0)), (1, 0)),
    "rotation_100": (lambda: make(216, 100, t=(0, 0, 0)), (0, None)),
    "forward_lowpar_100": (lambda: make(202, 100, t=(0, 0, 0.002), deg=0.0), (0, None)),
    "exact_64": (lambda: make(200, 64, noise=0.0), (None, None)),
    "min_8": (lambda: make(200, 8, noise=0.0, sets="perm", iterations=16), (0, None)),
    "wave_65": (lambda: make(200, 65), (None, None)),
    "wg_257": (lambda: make(202, 257, outliers=40, iterations=200), (None, None)),
    "wg_257_mt": (lambda: redraw_sets(case("wg_257"), 301), (None, None)),
    "unmatched_keys": (lambda: make(200, 100, extra1=200, extra2=180, outliers=10), (None, None)),
    "iter_1": (lambda: make(201, 80, iterations=1), (None, None)),
    "degenerate": (lambda: degenerate(213), (0, None)),
    "chunk_512": (lambda: make(203, 512, outliers=60, iterations=64), (1, 1)),
    "chunk_513": (lambda: make(202, 513, outliers=60, iterations=64), (1, 1)),
    "chunk_1025": (lambda: make(214, 1025, outliers=150, iterations=64), (1, 1)),
    "keys_1024_1025": (lambda: make(200, 100, extra1=924, extra2=925, outliers=10), (0, 1)),
    "keys_2049_3000": (lambda: make(200, 100, extra1=1949, extra2=2900, outliers=10), (0, 1)),
    "regrow_513": (lambda: make(205, 513, outliers=60, iterations=1100), (0, 1)),
}


def case(name):
    if name not in _cache:
        _cache[name] = CASES[name][0]()
    return _cache[name]


def reference(name):
    """the restatement's answer for a case, computed once and shared"""
    key = ("ref", name)
    if key not in _cache:
        sc = case(name)
        _cache[key] = R.initialize(sc["keys1"], sc["keys2"], sc["matches"], sc["sets"], sc["K4"], sc["sigma"], sc["min_parallax"], sc["min_triangulated"])
    return _cache[key]


def pack(sc):
    """the input file of tests/cpp/initializer_lockstep.cc"""
    return (np.array([len(sc["keys1"]), len(sc["keys2"]), len(sc["matches"]), sc["iterations"]], np.int32).tobytes() +
            np.array(list(sc["K4"]) + [sc["sigma"], sc["min_parallax"]], np.float32).tobytes() + np.int32(sc["min_triangulated"]).tobytes() +
            sc["keys1"].tobytes() + sc["keys2"].tobytes() + sc["matches"].tobytes() + sc["sets"].tobytes())


MARGIN = 1e-5       # relative distance of a comparison from its threshold below which a flag may differ between two float evaluations


def assert_conditions(name):
    """the conditions under which a scene is compared with the restatement, on the restatement's own trace"""
    sc, r = case(name), reference(name)
    assert r["margin_chi"] > MARGIN, "%s: a match of a winning hypothesis is %.2e from its chi-square threshold - choose another seed" % (name, r["margin_chi"])
    assert r["margin_rt"] > MARGIN, "%s: CheckRT compares %.2e from a threshold - choose another seed" % (name, r["margin_rt"])
    assert not abs(float(r["RH"]) - 0.40) <= 1e-4, "%s: RH = %r" % (name, r["RH"])
    assert r["ncand"] == 0 or abs(float(r["parallax"]) / sc["min_parallax"] - 1.0) > 1e-3, "%s: parallax %r" % (name, r["parallax"])
    assert not any(bool(e) for e in r.get("equalities", [])), "%s: an acceptance count is at equality" % name
    return sc, r
