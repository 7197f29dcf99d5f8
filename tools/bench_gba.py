"""One bundle adjustment of a loop-closure-sized map (orbb_global_bundle_adjustment: the blocked reduced-system path, k_gba_*) at
40 / 160 / 1000 keyframes, beside Optimizer::BundleAdjustment's dense path (orbb_bundle_adjustment) where that path is usable.

  python tools/bench_gba.py                                # 40:4000 and 160:16000 with both paths, 1000:100000 with the new one only
  python tools/bench_gba.py 160:16000 --calls 10 --warm 3  # keyframes : points
  python tools/bench_gba.py 1000:100000 --new-only --calls 3 --warm 1
  rocprofv3 --kernel-trace --stats -- python tools/bench_gba.py 1000:100000 --new-only --calls 1 --warm 1      # the kernels apart

Scene: a vectorised form of tests/gba_scene.py's window scene (keyframes along x at 2 m steps looking down +z, points 4 to 20 m deep
along the whole path, the last four keyframes back at the start, keyframe 0 fixed, half the observations stereo, 0.7 px noise scaled
by the level), 10 iterations without the Huber kernel as LoopClosing::RunGlobalBundleAdjustment asks.  The old path is never run past
--old-limit keyframes (default 200): its Schur kernel starts nf^2 workgroups over a [nf][P] table and ONE workgroup factorises.
The figure is the median (and the minimum) of a host clock around the synchronous call, which ends in a stream synchronisation:
staging, the host's pattern building, the per-trial synchronisations and the runtime's calls included.  `set-up` is the same clock
around a call with 0 iterations - argument checks, layout, staging, upload, the round's columns and, on the new path, the block
pattern and its upload, then the outputs - so the difference of the two paths' set-ups is what the pattern costs the host per call;
at sizes where the old path is not run the new path's whole set-up is reported.  Launches come from the call's own record.
There is no g2o build on this hardware: no speed-up over the reference is claimed.  One JSON line per size and path."""
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gba_scene as GS       # noqa: E402
import lba_ref as R          # noqa: E402
import lba_scene as S        # noqa: E402

args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name)
        v = int(args[i + 1])
        del args[i:i + 2]
        return v
    return default


CALLS, WARM, OLD_LIMIT = opt("--calls", 10), opt("--warm", 3), opt("--old-limit", 200)
new_only = "--new-only" in args
if new_only:
    args.remove("--new-only")
sizes = [tuple(int(x) for x in a.split(":")) for a in args] or [(40, 4000), (160, 16000), (1000, 100000)]
pkg = importlib.import_module("orb_slam2v2-1_amd")


def make(seed, nkf, npts, nloop=4, noise=0.7, rot=0.01, trans=0.05, ptnoise=0.08):
    """gba_scene.make without its per-observation loop: visibility as one [points, keyframes] mask per chunk of points"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy, bf = S.CAM
    xs = GS.STEP * np.arange(nkf, dtype=np.float64)
    xs[nkf - nloop:] = GS.STEP * (np.arange(nloop) + 0.5)
    Ts = np.tile(np.eye(4), (nkf, 1, 1))
    for i in range(nkf):
        Twc = np.eye(4)
        Twc[:3, :3] = S.rodrigues([0.0, rng.normal(0, 0.01), 0.0])
        Twc[:3, 3] = [xs[i] + rng.normal(0, 0.05), rng.normal(0, 0.05), rng.normal(0, 0.05)]
        Ts[i] = np.linalg.inv(Twc)
    span = GS.STEP * (nkf - nloop - 1)
    z = rng.uniform(4.0, 20.0, npts)
    Xw = np.stack([np.sort(rng.uniform(-3.0, span + 3.0, npts)), rng.uniform(-0.12, 0.12, npts) * z, z], 1)
    parts = []
    for a in range(0, npts, 4096):
        X = Xw[a:a + 4096]
        Xc = np.einsum("kij,pj->pki", Ts[:, :3, :3], X) + Ts[None, :, :3, 3]
        u, v = fx * Xc[..., 0] / Xc[..., 2] + cx, fy * Xc[..., 1] / Xc[..., 2] + cy
        p, k = np.nonzero((Xc[..., 2] > 0.5) & (u > 0) & (u < S.W) & (v > 0) & (v < S.H))
        parts.append((p + a, k, u[p, k], v[p, k], Xc[p, k, 2]))
    p, k, u, v, zc = (np.concatenate(c) for c in zip(*parts))
    n = len(p)
    oc = rng.integers(0, S.NLEVELS, n)
    sig = noise * S.SF[oc].astype(np.float64)
    uu, vv = u + rng.normal(0, 1, n) * sig, v + rng.normal(0, 1, n) * sig
    ur = np.where(rng.random(n) < 0.5, uu - bf / zc + rng.normal(0, 1, n) * sig, -1.0)
    ur[ur < 0] = -1.0
    keep = np.bincount(p, minlength=npts) >= 2
    renum = np.cumsum(keep) - 1
    sel = keep[p]
    obs = np.zeros(int(sel.sum()), R.OBS_DTYPE)
    obs["kf"], obs["pt"], obs["u"], obs["v"], obs["ur"], obs["inv_sigma2"] = k[sel], renum[p[sel]], uu[sel], vv[sel], ur[sel], S.INV_SIGMA2[oc[sel]]
    Xw = Xw[keep]
    kfs = np.zeros(nkf, R.KF_DTYPE)
    for i in range(nkf):
        T = Ts[i].copy()
        if i > 0:
            d = np.eye(4)
            d[:3, :3] = S.rodrigues(rng.normal(0, rot, 3))
            d[:3, 3] = rng.normal(0, trans, 3)
            T = d @ T
        kfs["Tcw"][i] = T.astype(np.float32).reshape(-1)
    kfs["fixed"][0] = 1
    kfs["fx"], kfs["fy"], kfs["cx"], kfs["cy"], kfs["bf"] = fx, fy, cx, cy, bf
    pts = np.zeros(len(Xw), R.PT_DTYPE)
    X0 = Xw + rng.normal(0, ptnoise, Xw.shape)
    pts["x"], pts["y"], pts["z"] = X0[:, 0], X0[:, 1], X0[:, 2]
    return dict(kfs=kfs, pts=pts, obs=obs)


def timed(fn, calls, warm):
    ms, res = [], None
    for _ in range(warm + calls):
        t0 = time.perf_counter()
        res = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = ms[warm:]
    return float(np.median(ms)), float(min(ms)), res


for nkf, npts in sizes:
    sc = make(1000 + nkf, nkf, npts)
    K, P, E = len(sc["kfs"]), len(sc["pts"]), len(sc["obs"])
    paths = [("blocked", lambda it: pkg.global_bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], iterations=it, robust=False))]
    if not new_only and nkf <= OLD_LIMIT:
        paths.insert(0, ("dense", lambda it: pkg.bundle_adjustment(sc["kfs"], sc["pts"], sc["obs"], iterations=it, robust=False)))
    line = {}
    for name, call in paths:
        med, mn, res = timed(lambda: call(GS.ITERATIONS), CALLS, WARM)
        setup, setup_min, _ = timed(lambda: call(0), max(3, CALLS // 2), 1)
        info = res[3]
        line[name] = dict(path=name, keyframes=K, points=P, observations=E, calls=CALLS, median_ms=round(med, 3), min_ms=round(mn, 3),
                          setup_median_ms=round(setup, 3), setup_min_ms=round(setup_min, 3), iterations=info["iterations"][0], trials=info["trials"][0],
                          free_poses=info["free_poses"][0])
        if name == "blocked":
            line[name].update(blocks=info["blocks"][0], panels=info["panels"][0], contributions=info["contributions"][0], launches=info["launches"])
        print(json.dumps(line[name]), flush=True)
    if len(line) == 2:
        d, b = line["dense"], line["blocked"]
        allow = max(d["median_ms"] - d["min_ms"], b["median_ms"] - b["min_ms"])
        print(json.dumps(dict(keyframes=K, points=P, blocked_over_dense=round(b["median_ms"] / d["median_ms"], 4), allowance_ms=round(allow, 3),
                              blocked_not_slower=bool(b["median_ms"] <= d["median_ms"] + allow),
                              pattern_ms=round(b["setup_median_ms"] - d["setup_median_ms"], 3))), flush=True)
