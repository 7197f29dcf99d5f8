"""The local map (orbt_localmap_set_map, orbt_update_local_map) on one map, beside the same computation on the CPU.

  python tools/bench_localmap.py                      # 500 keyframes x 2000 features
  python tools/bench_localmap.py --keyframes 60 --calls 50 --warm 5
  rocprofv3 --kernel-trace --stats -- python tools/bench_localmap.py --calls 5 --warm 2      # the kernels apart, in a run of its own

The map: K keyframes along a path with 2000 features each, about 10 observations per point, the spanning tree a chain, every
keyframe's covisible list its 20 nearest neighbours by distance; the frame: the 2000 points of the middle keyframe, 30 % of the slots
empty.  Reported: `set_map_ms` and `snapshot_bytes` (the host clock around the C entry point: checks, packing, one upload, one
synchronisation) and what that is per keyframe insertion if the snapshot is rebuilt after each (`set_map_ms` itself: one rebuild per
insertion); the median and minimum of `update` (a host clock around orbt_update_local_map through ctypes with its arrays made once);
`upload_ms` / `download_ms`: copies of exactly the call's input and output bytes between pinned memory and the device, timed alone,
and `launches_ms` = median - upload - download: what is left for the launches and the two synchronisations (`launches`, `syncs` from
the call's info); `host_*_ms`: the same rules as pointer-walking std::map / std::set loops over host/frame_shim.h's objects
(tools/localmap_host_loops.cc, g++ -O2, one thread, the same map on the same machine, the best of 5).  The two sides are checked to
agree on what they computed before a number is printed.  No ratio is a goal here.  One JSON line."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
args = sys.argv[1:]


def opt(name, default):
    if name in args:
        i = args.index(name)
        v = int(args[i + 1])
        del args[i:i + 2]
        return v
    return default


CALLS, WARM, K, FEATS = opt("--calls", 30), opt("--warm", 5), opt("--keyframes", 500), opt("--features", 2000)
pkg = importlib.import_module("orb_slam2v2-1_amd")
SF = np.array([1.2 ** l for l in range(8)], np.float32)


def make(seed, K, feats, mean_obs):
    """a point is seen by a run of neighbouring keyframes around a random centre; feature index = rank of the observation inside its
    keyframe, so every keyframe has about `feats` features, all of them naming a point"""
    rng = np.random.default_rng(seed)
    P = K * feats // mean_obs
    kf = np.zeros(K, pkg.COVIS_KEYFRAME_DTYPE)
    kf["id"] = np.arange(K)
    n = np.clip(rng.poisson(mean_obs - 2, P) + 2, 2, K)
    first = np.clip(rng.integers(0, K, P) - n // 2, 0, K - n)
    pt_of = np.repeat(np.arange(P), n)
    kf_of = np.repeat(first, n) + (np.arange(len(pt_of)) - np.repeat(np.cumsum(n) - n, n))
    order = np.lexsort((pt_of, kf_of))
    idx = np.empty(len(pt_of), np.int64)
    start = np.searchsorted(kf_of[order], np.arange(K))
    idx[order] = np.arange(len(pt_of)) - start[kf_of[order]]
    pts = np.zeros(P, pkg.COVIS_POINT_DTYPE)
    pts["pos"] = np.stack([2.0 * (first + n / 2.0), rng.uniform(-2, 2, P), rng.uniform(4, 20, P)], 1)
    pts["ref_kf"] = first
    pts["bad"] = rng.random(P) < 0.01
    table = pkg.covis_table(kf, pts, np.stack([pt_of, kf_of, idx, np.zeros_like(idx), np.zeros_like(idx)], 1), SF)
    fl = []
    for s in range(K):
        m = kf_of == s
        f = np.zeros(int(m.sum()), pkg.COVIS_FEATURE_DTYPE)
        f["point"][idx[m]] = pt_of[m]
        fl.append(f)
    features = pkg.covis_queries(np.arange(K), fl)
    cov = [[c for d in range(1, 11) for c in (s - d, s + d) if 0 <= c < K] for s in range(K)]
    graph = pkg.localmap_graph(np.arange(-1, K - 1), cov, [[s + 1] if s + 1 < K else [] for s in range(K)])
    views = np.zeros(P, pkg.LOCALMAP_VIEW_DTYPE)
    views["normal"] = rng.normal(size=(P, 3))
    views["max_distance"], views["min_distance"], views["observations"] = rng.uniform(5, 9, P), rng.uniform(0.1, 1, P), n
    desc = rng.integers(0, 256, (P, 32), dtype=np.uint8)
    frame = fl[K // 2]["point"].copy()
    frame[rng.random(len(frame)) < 0.3] = -1
    return table, features, graph, views, desc, frame.astype(np.int32)


def timed(fn, calls=CALLS, warm=WARM):
    ms = []
    for _ in range(warm + calls):
        t0 = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    ms = ms[warm:]
    return float(np.median(ms)), float(min(ms))


def copy_ms(nbytes, down):
    import torch
    h = torch.empty(max(nbytes, 1), dtype=torch.uint8).pin_memory()
    d = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    st = torch.cuda.Stream()

    def go():
        with torch.cuda.stream(st):
            (h if down else d).copy_(d if down else h, non_blocking=True)
        st.synchronize()
    return timed(go)[0]


def al(n):
    return (n + 255) & ~255


table, features, graph, views, desc, frame = make(7, K, FEATS, 10)
P, N = len(table["pts"]), len(frame)
L = pkg.lib()
lm = pkg.LocalMap()
ct, cq = pkg._covis_c_table(table), pkg._covis_c_queries(features)
cm = pkg.LocalMapMap(C.addressof(ct), C.addressof(cq), *[graph[k].ctypes.data for k in ("parent", "cov_off", "cov", "child_off", "child")], views.ctypes.data,
                     desc.ctypes.data)


def set_map():
    rc = L.orbt_localmap_set_map(lm._h, C.addressof(cm))
    if rc:
        raise pkg.OrbxError(rc, L.orbx_last_error().decode())


set_ms = timed(set_map, calls=5, warm=1)
lm.K, lm.P = K, P
info = lm.info()
o = {"frame_points": np.empty(N, np.int32), "holder": np.empty(N, np.int32), "ext_obs": np.empty(N, np.int32), "local_kf": np.empty(K, np.int32),
     "local_pts": np.empty(P, np.int32), "pts": np.empty(P, pkg.WORLDPOINT_DTYPE), "mp_desc": np.empty((P, 32), np.uint8)}
res = pkg.LocalMapResult(*[o[k].ctypes.data for k in ("frame_points", "holder", "ext_obs", "local_kf", "local_pts", "pts", "mp_desc")])


def update():
    rc = L.orbt_update_local_map(lm._h, frame.ctypes.data, N, None, 0, 80, 10, C.addressof(res))
    if rc:
        raise pkg.OrbxError(rc, L.orbx_last_error().decode())


upd = timed(update)
nk, m = res.n_local_kf, res.n_local_pts
in_bytes = al(N * 12)
out_bytes = al(32) + 3 * al(4 * N) + al(4 * nk) + al(4 * m) + al(40 * m) + al(32 * m)
up, down = copy_ms(in_bytes, False), copy_ms(out_bytes, True)

with tempfile.TemporaryDirectory() as tmp:
    exe = os.path.join(tmp, "localmap_host_loops")
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "orb_slam2v2-1_amd", "host"),
                           os.path.join(ROOT, "tools", "localmap_host_loops.cc"), "-o", exe])
    hd = np.array([K, P, len(table["obs"]), len(SF), len(features["feat"]), len(graph["cov"]), len(graph["child"]), N, 0, 80, 10], np.int32)
    with open(os.path.join(tmp, "in.bin"), "wb") as f:
        for a in (hd, table["kf"], table["pts"], table["obs_off"], table["obs"], table["sf"], features["feat_off"], features["feat"], graph["parent"],
                  graph["cov_off"], graph["cov"], graph["child_off"], graph["child"], views, desc, frame):
            f.write(a.tobytes())
    host = json.loads(subprocess.run([exe, os.path.join(tmp, "in.bin"), "5"], check=True, capture_output=True, text=True).stdout)

# the two sides computed the same thing
lp = o["local_pts"][:m].astype(np.int64)
assert (nk, m, int(res.info[2])) == (host["n_local_kf"], host["n_local_pts"], host["ref_kf"]), (nk, m, tuple(res.info), host)
assert int((lp * (np.arange(m) % 7 + 1)).sum()) == host["points_sum"], host
hs = int(o["holder"][o["holder"] != -1].sum())
assert hs == host["holder_sum"], (hs, host)
line = dict(keyframes=K, points=P, features=len(features["feat"]), observations=len(table["obs"]), frame_points=N, calls=CALLS,
            set_map_ms=round(set_ms[0], 3), set_map_min_ms=round(set_ms[1], 3), snapshot_bytes=info["snapshot_bytes"], device_bytes=info["device_bytes"],
            update_median_ms=round(upd[0], 4), update_min_ms=round(upd[1], 4), upload_ms=round(up, 4), download_ms=round(down, 4),
            launches_ms=round(upd[0] - up - down, 4), input_bytes=in_bytes, output_bytes=out_bytes, launches=int(res.info[5]), syncs=int(res.info[6]),
            n_local_kf=nk, n_local_pts=m, n_voted=int(res.info[1]), extension_end=int(res.info[4]))
line.update({k: round(v, 4) for k, v in host.items() if k.endswith("_ms")})
line["host_total_ms"] = round(sum(v for k, v in host.items() if k.endswith("_ms")), 4)
print(json.dumps(line), flush=True)
lm.close()
