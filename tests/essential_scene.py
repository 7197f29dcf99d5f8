"""Seeded Optimizer::OptimizeEssentialGraph scenes: keyframes on an arc of a circle looking along it, a map that drifted along the
spanning tree (rotation, translation and - for the monocular cases - scale), the last keyframes of a branch carrying a
CorrectedSim3 (where the loop says they are) and a NonCorrectedSim3 (where the drifted map had them), as LoopClosing::CorrectLoop
leaves them (src/LoopClosing.cc:430-470); spanning-tree, covisibility (band) and loop-connection edges; two map points per keyframe."""
import numpy as np

import essential_ref as R

MARGIN = 1e-5       # relative distance from a branch threshold below which a branch may differ; the value tests/lba_scene.py uses
DRAWS = 16


def rodrigues(rvec):
    rvec = np.asarray(rvec, np.float64)
    th = np.linalg.norm(rvec)
    K = np.array([[0, -rvec[2], rvec[1]], [rvec[2], 0, -rvec[0]], [-rvec[1], rvec[0], 0]])
    return np.eye(3) if th == 0 else np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def sim3_of(T, s=1.0):
    """4x4 Tcw, scale -> (q [1, 4], t [1, 3], s [1]): Sim3(R, s * t, s)"""
    T = np.asarray(T, np.float64)
    return R.quat_from_R(T[None, :3, :3]), s * T[None, :3, 3], np.array([float(s)])


def make(seed, n, parents=None, band=1, fixed=0, groups=(), loops=(), extra=(), fix_scale=True, rot=0.004, trans=0.01, sd=0.0, arc=None,
         angle=None, group_rot=0.0, group_scale=None, group_pure=None, group_bend=0.0):
    """-> dict(vertices, edges, points, fix_scale, true_centres [n, 3], drift_centres [n, 3]).
    parents [n]: the spanning tree (default: a chain, parent i - 1; -1: none).  band: covisibility edges (i, i - d), d = 2..band.
    fixed: the fixed vertex (None: none).  groups: lists of vertices that carry Corrected / NonCorrected entries, each group moved
    rigidly with its LAST member, which goes to its true pose (with the drifted map's scale there).  loops: (i, j) kind-0 edges;
    extra: (i, j, kind) further edges.  rot / trans: drift per tree edge (rad, m); sd: log scale drift per tree edge.
    angle [n]: the angle of every keyframe on the circle (default: evenly over `arc`, a full turn less one step).
    group_rot: a further rotation (rad) of every group's corrected poses, so that the edges into the group start with a large angle.
    group_scale: per group a scale in place of the drifted map's (None: that one).  group_pure: per group, True: the group keeps its
    drifted pose and only takes the scale (an edge into it then starts with an error of scale and translation alone).  group_bend: a
    rotation (rad) of every member but the last against the group, so that Scw[j] * Scw[i]^-1 inside a group is not Snc[j] * Snc[i]^-1."""
    rng = np.random.default_rng(seed)
    parents = np.array([i - 1 for i in range(n)] if parents is None else parents)
    if angle is None:
        arc = 2 * np.pi * n / (n + 1) if arc is None else arc
        angle = arc * np.arange(n) / n
    rad = 8.0
    Twc = np.zeros((n, 4, 4))
    for i in range(n):
        a = angle[i]
        Twc[i] = np.eye(4)
        Twc[i, :3, :3] = rodrigues([0.0, -a, 0.0])
        Twc[i, :3, 3] = [rad * np.sin(a), 0.05 * np.sin(3 * a), rad * (1 - np.cos(a))]
    Td = np.zeros_like(Twc)       # the drifted map
    depth = np.zeros(n, np.int64)
    for i in range(n):
        p = parents[i]
        if p < 0:
            Td[i] = Twc[i]
            continue
        assert p < i
        depth[i] = depth[p] + 1
        rel = np.linalg.inv(Twc[p]) @ Twc[i]
        rel[:3, 3] *= np.exp(sd * depth[i])
        rel[:3, 3] += rng.normal(0, trans, 3)
        rel[:3, :3] = rel[:3, :3] @ rodrigues(rng.normal(0, rot, 3))
        Td[i] = Td[p] @ rel
    vt = np.zeros(n, R.VERTEX_DTYPE)
    S = [sim3_of(np.linalg.inv(Td[i])) for i in range(n)]
    for i in range(n):
        for f, v in zip(("q", "t", "s"), S[i]):
            vt["Scw"][f][i] = v[0]
            vt["Snc"][f][i] = v[0]
    for gi, g in enumerate(groups):
        a = g[-1]
        s = 1.0 if fix_scale else float(np.exp(sd * depth[a]))
        if group_scale is not None and group_scale[gi] is not None:
            s = float(group_scale[gi])
        pure = group_pure is not None and group_pure[gi]
        Ta = np.linalg.inv(Td[a] if pure else Twc[a])
        if group_rot and not pure:
            Ta[:3, :3] = rodrigues([0.3 * group_rot, group_rot, -0.2 * group_rot]) @ Ta[:3, :3]
        Sa = sim3_of(Ta, s)
        for i in g:
            Tic = np.linalg.inv(Td[i]) @ Td[a]
            if group_bend and i != a:
                Tic[:3, :3] = rodrigues([group_bend, -0.5 * group_bend, 0.25 * group_bend]) @ Tic[:3, :3]
            Sic = sim3_of(Tic)
            Sc = R.mul(Sic, Sa)
            for f, v in zip(("q", "t", "s"), Sc):
                vt["Scw"][f][i] = v[0]
            vt["has_nc"][i] = 1
    if fixed is not None:
        vt["fixed"][fixed] = 1
    edges = [(i, j, 0) for i, j in loops]
    for i in range(n):
        if parents[i] >= 0:
            edges.append((i, int(parents[i]), 1))
        for d in range(2, band + 1):
            if i - d >= 0:
                edges.append((i, i - d, 1))
    edges += [tuple(e) for e in extra]
    ed = np.array(edges, R.EDGE_DTYPE) if edges else np.zeros(0, R.EDGE_DTYPE)
    pts = np.zeros(2 * n, R.POINT_DTYPE)
    for p in range(2 * n):
        i = p // 2
        Xc = np.array([rng.uniform(-1, 1), rng.uniform(-0.5, 0.5), rng.uniform(2, 6), 1.0])
        Xw = Td[i] @ Xc
        pts["x"][p], pts["y"][p], pts["z"][p], pts["ref"][p] = Xw[0], Xw[1], Xw[2], i
    return dict(vertices=vt, edges=ed, points=pts, fix_scale=bool(fix_scale), true_centres=Twc[:, :3, 3].copy(), drift_centres=Td[:, :3, 3].copy())


def _ring(n, band, seed, fix_scale, sd=0.0, **kw):
    return dict(seed=seed, n=n, band=band, groups=[list(range(n - 5, n))], loops=[(i, j) for i in (n - 1, n - 2) for j in (0, 1, 2)],
                fix_scale=fix_scale, sd=sd, **kw)


# The shapes the tests run, smallest where the kernels can go wrong: name -> make() arguments.  No kernel stages a column in LDS
# under a bound (csrc/orbx_essential.hip keeps only the 7x7 diagonal block there), so no case sits on either side of one; the
# constants that choose a path are the 256 threads of a workgroup (wide: 316 edges, 80 vertices x 7 rows and 49-entry blocks on
# both sides of it) and the 16 slots of an edge.
# The Levenberg branches (optimization_algorithm_levenberg.cpp:100-161; tests/test_lm_branches_cpu.py counts them): every case
# accepts one trial per iteration until it ends.  The fixed-scale cases end by ten rejected trials whose rho is rounding noise;
# ring_free_scale, branches and ring_rejected by ten rejected trials with |rho| far above it (ring_rejected: [1, 1, 10], rho from
# -1.2 to -0.23, after two accepted steps - so `iterations=2` and `iterations=3` must leave the same estimates); ring_nbad by three
# iterations of negligible gain (ORBG_END_NBAD, trials [1, 1, 1, 1, 1], every |rho| >= 3.6e-5).
CASES = {
    "chain": dict(seed=701, n=12, groups=[[10, 11]]),
    "ring_fixed_scale": _ring(24, 3, 752, True),
    "ring_free_scale": _ring(24, 3, 703, False, sd=0.002),
    "clique": dict(seed=704, n=6, band=5, groups=[[4, 5]], arc=1.0),
    "two_branches": dict(seed=705, n=11, parents=[-1, 0, 1, 2, 3, 4, 0, 6, 7, 8, 9], groups=[[5], [9, 10]],
                         angle=[0.0] + [0.25 * k for k in range(1, 6)] + [-0.25 * k for k in range(1, 6)]),
    "fixed_mid": dict(seed=706, n=12, band=2, fixed=6, groups=[[10, 11]]),
    "dup_pair": dict(seed=707, n=8, groups=[[6, 7]], extra=[(5, 4, 1), (3, 2, 1), (3, 2, 1)]),
    "kinds": dict(seed=818, n=10, band=2, groups=[[7, 8, 9]], loops=[(9, 0), (9, 8)], extra=[(9, 8, 1)], group_bend=0.01),
    "wide": _ring(80, 4, 759, True, rot=0.002, trans=0.005),
    "branches": dict(seed=710, n=11, parents=[-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 0], extra=[(i, i - 2, 1) for i in range(2, 10)],
                     groups=[[3], [6], [8, 9], [10]], group_scale=[1.0, None, None, 1.02], group_pure=[False, False, False, True],
                     fix_scale=False, sd=0.004, group_rot=0.05, angle=[0.3 * k for k in range(10)] + [-0.3]),
    "ring_nbad": _ring(24, 3, 752, True, group_rot=0.5),
    "ring_rejected": _ring(24, 3, 703, False, sd=0.002, group_rot=3.0),
}
_cache, _refs = {}, {}


def case(name):
    if name not in _cache:
        _cache[name] = make(**CASES[name])
    return _cache[name]


def run(sc, **kw):
    return R.optimize(sc["vertices"], sc["edges"], sc["points"], sc["fix_scale"], **kw)


def reference(name):
    """-> (scene, the restatement's result, its DRAWS results with every sum over edges and vertices in a random order and every
    sin / cos / acos / log / exp moved by up to +-2 ulp, S: its largest deviation in the double estimates over those).  Computed
    once, shared by the CPU and the GPU tests."""
    if name not in _refs:
        sc = case(name)
        ref = run(sc)
        rng = np.random.default_rng(4321)
        draws = [run(sc, order=rng, perturb=rng) for _ in range(DRAWS)]
        dev = max([0.0] + [float(np.abs(d["est"] - ref["est"]).max()) for d in draws])
        _refs[name] = (sc, ref, draws, dev)
    return _refs[name]


_cuts = {}


def reference_cut(name, iterations):
    """reference() for a call cut short after `iterations` iterations: S is the spread of THAT run over its 16 draws"""
    if (name, iterations) not in _cuts:
        sc = case(name)
        ref = run(sc, iterations=iterations)
        rng = np.random.default_rng(4321)
        draws = [run(sc, order=rng, perturb=rng, iterations=iterations) for _ in range(DRAWS)]
        dev = max([0.0] + [float(np.abs(d["est"] - ref["est"]).max()) for d in draws])
        _cuts[(name, iterations)] = (sc, ref, draws, dev)
    return _cuts[(name, iterations)]
